"""Host-side (no GPU) checks of the prioritised replay draw's ABI (include/reacher_replay_priority.h):
every declared rd_replay_prio_* name is exported and registered, the ctypes mirror matches the header
field by field, every argument check answers RD_EINVAL before any device call (there is no GPU here, so
an answer at all is the proof), both drivers take ``replay_priority``, and the model the GPU tests
compare against (tests/replay_prio_model.py) is consistent with itself and follows the weights.

Handles: the checks that need no handle get a fake non-NULL pointer that a rejected call never
dereferences; "priorities not enabled" and "capacity" read the handle, so they get zeroed host memory
(a handle with capacity 0 and priorities off) or the same with its first member, the capacity, set.
The checks behind an ENABLED handle (windows > max_batch, a ring never pushed to, a second enable) are
in tests/test_replay_prio_gpu.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.replay_model import REC, STEPS
from tests.replay_prio_model import ERR, INIT_CONST, INIT_RECORD, PRIO_MAX, SQERR, PrioRingModel, clamp, quantise

HEADER = "reacher_replay_priority.h"
RD_EINVAL = -100000
NAMES = ["rd_replay_prio_enable", "rd_replay_prio_configure", "rd_replay_prio_enabled", "rd_replay_prio_table",
         "rd_replay_prio_fill", "rd_replay_prio_update_rows", "rd_replay_prio_update_windows",
         "rd_replay_prio_sample_rows", "rd_replay_prio_sample_windows"]


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, replay  # noqa: F401  (replay registers the symbols)
    build.build(verbose=False)
    return _native.load()


def _header():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_every_declared_name_is_exported_with_a_signature(lib):
    from reacherdistilation_amd import _native
    names = sorted(set(re.findall(r"\b(rd_replay_prio_[a-z0-9_]+)\s*\(", _header())))
    assert names == sorted(NAMES)
    assert '#include "reacher_replay.h"' in _header()
    have = _native.exported_symbols()
    for name in names:
        assert have.get(name) is True, name
        assert getattr(lib, name).argtypes is not None, name


def test_ctypes_mirror_matches_the_header():
    from reacherdistilation_amd.replay import RdReplayPrioConfig as C
    fields = [f[0] for f in C._fields_]
    body = re.search(r"typedef struct \{([^}]*)\}\s*rd_replay_prio_config;", _header()).group(1)
    assert fields == re.findall(r"(\w+)\s*(?:,|;)", body)   # same members, same order
    lines = "\n".join(f'printf("{f} %zu\\n", offsetof(rd_replay_prio_config, {f}));' for f in fields)
    src = (f'#include <stddef.h>\n#include <stdio.h>\n#include "{HEADER}"\n'
           f'int main(void) {{ printf("sizeof %zu\\n", sizeof(rd_replay_prio_config)); {lines} return 0; }}\n')
    d = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(d, exist_ok=True)
    c, exe = os.path.join(d, "layout_rd_replay_prio_config.c"), os.path.join(d, "layout_rd_replay_prio_config")
    with open(c, "w") as fh:
        fh.write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    lay = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert lay["sizeof"] == ctypes.sizeof(C) == 24
    for f in fields:
        assert lay[f] == getattr(C, f).offset, f


def test_constants_match_the_header():
    from reacherdistilation_amd import replay
    txt = _header()
    for name, value in (("RD_REPLAY_PRIO_MAX", replay.PRIO_MAX), ("RD_REPLAY_PRIO_MAX_CAPACITY", replay.PRIO_MAX_CAPACITY),
                        ("RD_REPLAY_PRIO_SCAN_TILE", replay.PRIO_SCAN_TILE), ("RD_PRIO_SQERR", replay.PRIO_SQERR),
                        ("RD_PRIO_ERR", replay.PRIO_ERR), ("RD_PRIO_INIT_CONST", replay.PRIO_INIT_CONST),
                        ("RD_PRIO_INIT_RECORD", replay.PRIO_INIT_RECORD)):
        assert re.search(rf"#define {name} {value}\b", txt), name
    assert (replay.PRIO_MAX, replay.PRIO_MAX_CAPACITY) == (16777216, 4194304) == (PRIO_MAX, 1 << 22)
    assert (replay.PRIO_SQERR, replay.PRIO_ERR, replay.PRIO_INIT_CONST, replay.PRIO_INIT_RECORD) == (0, 1, 0, 1)
    assert (SQERR, ERR, INIT_CONST, INIT_RECORD) == (0, 1, 0, 1)


# -- argument checks --------------------------------------------------------------------------
def _msg(lib):
    return lib.rd_last_error().decode()


FAKE = ctypes.c_void_p(0x1000)   # a non-NULL handle that a rejected call never dereferences


def _zero_handle(capacity=0):
    """Zeroed host memory read as a handle: priorities off; `capacity` is the struct's first member."""
    raw = (ctypes.c_int64 * 64)()
    raw[0] = capacity
    return raw, ctypes.c_void_p(ctypes.addressof(raw))


def _buffers(n=7):
    """Host memory standing in for device buffers (never dereferenced), 64-byte aligned."""
    raw = (ctypes.c_char * (64 * (n + 1)))()
    base = (ctypes.addressof(raw) + 63) & ~63
    return raw, [ctypes.c_void_p(base + 64 * k) for k in range(n)]


def _sample(**kw):
    from reacherdistilation_amd.replay import RdReplaySample
    s = RdReplaySample(steps=10, start_mode=0, windows=4, window_base=0, recent=0, seed=1)
    for k, v in kw.items():
        setattr(s, k, v)
    return ctypes.byref(s)


def _config(**kw):
    from reacherdistilation_amd.replay import RdReplayPrioConfig
    c = RdReplayPrioConfig(measure=0, shift=16, q_min=1, q_init=1 << 24, init_mode=0, reserved=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return ctypes.byref(c)


BAD_CONFIG = [("measure", 2), ("measure", -1), ("shift", -1), ("shift", 25), ("q_min", 0), ("q_min", 2 ** 24 + 1),
              ("q_init", 0), ("q_init", 2 ** 24 + 1), ("init_mode", 2), ("init_mode", -1), ("reserved", 1)]


@pytest.mark.parametrize("fn", ["rd_replay_prio_enable", "rd_replay_prio_configure"])
def test_config_calls_reject_bad_arguments_before_any_device_call(lib, fn):
    raw, (table, *_r) = _buffers()
    extra = (table,) if fn.endswith("enable") else ()
    assert getattr(lib, fn)(None, _config(), *extra) == RD_EINVAL
    assert fn + ":" in _msg(lib) and "null handle" in _msg(lib)
    assert getattr(lib, fn)(FAKE, None, *extra) == RD_EINVAL
    assert fn + ":" in _msg(lib) and "null config" in _msg(lib)
    for field, value in BAD_CONFIG:                      # before the handle is read: FAKE is never touched
        assert getattr(lib, fn)(FAKE, _config(**{field: value}), *extra) == RD_EINVAL, (field, value)
        assert fn + ":" in _msg(lib) and field in _msg(lib), (field, value, _msg(lib))
    del raw


def test_enable_rejects_a_ring_above_the_capacity_limit(lib):
    raw, (table, *_r) = _buffers()
    mem, h = _zero_handle(capacity=2 ** 22 + 1)
    assert lib.rd_replay_prio_enable(h, _config(), table) == RD_EINVAL
    assert "rd_replay_prio_enable:" in _msg(lib) and "capacity" in _msg(lib)
    del raw, mem


def test_configure_and_fill_need_enabled_priorities(lib):
    mem, h = _zero_handle()
    assert lib.rd_replay_prio_configure(h, _config()) == RD_EINVAL
    assert "rd_replay_prio_configure:" in _msg(lib) and "not enabled" in _msg(lib)
    assert lib.rd_replay_prio_fill(None, 5) == RD_EINVAL and "null handle" in _msg(lib)
    for q in (0, 2 ** 24 + 1):
        assert lib.rd_replay_prio_fill(FAKE, q) == RD_EINVAL
        assert "rd_replay_prio_fill:" in _msg(lib) and "q " in _msg(lib)
    assert lib.rd_replay_prio_fill(h, 5) == RD_EINVAL and "not enabled" in _msg(lib)
    assert lib.rd_replay_prio_enabled(None) == -1 and lib.rd_replay_prio_enabled(h) == 0
    assert lib.rd_replay_prio_table(None) is None and lib.rd_replay_prio_table(h) is None
    del mem


def test_updates_reject_bad_arguments_before_any_device_call(lib):
    raw, (idx, s, *_r) = _buffers()
    mem, h = _zero_handle()
    rows, win = "rd_replay_prio_update_rows", "rd_replay_prio_update_windows"
    cases = [(rows, (None, idx, s, 4), "null handle"), (rows, (FAKE, None, s, 4), "null idx"),
             (rows, (FAKE, idx, None, 4), "null s_pdflat"), (rows, (FAKE, idx, s, 0), "rows"),
             (rows, (FAKE, idx, s, -3), "rows"), (rows, (h, idx, s, 4), "not enabled"),
             (win, (None, idx, s, 10, 4), "null handle"), (win, (FAKE, None, s, 10, 4), "null idx"),
             (win, (FAKE, idx, None, 10, 4), "null s_pdflat"), (win, (FAKE, idx, s, 0, 4), "steps"),
             (win, (FAKE, idx, s, 51, 4), "steps"), (win, (FAKE, idx, s, -1, 4), "steps"),
             (win, (FAKE, idx, s, 10, 0), "windows"), (win, (FAKE, idx, s, 10, -2), "windows"),
             (win, (h, idx, s, 10, 4), "not enabled")]
    for fn, args, word in cases:
        assert getattr(lib, fn)(*args) == RD_EINVAL, (fn, word)
        assert fn + ":" in _msg(lib) and word in _msg(lib), (fn, word, _msg(lib))
    del raw, mem


def test_sample_windows_rejects_bad_arguments_before_any_device_call(lib):
    raw, (ob, pv, tw, pr, idx, prob, _) = _buffers()
    mem, h = _zero_handle()
    fn = lib.rd_replay_prio_sample_windows
    cases = [((None, _sample(), ob, pv, tw, pr, idx, prob), "null handle"),
             ((FAKE, None, ob, pv, tw, pr, idx, prob), "null sample"),
             ((FAKE, _sample(), None, pv, tw, pr, idx, prob), "null ob_w"),
             ((FAKE, _sample(), ob, None, tw, pr, idx, prob), "null prev_w"),
             ((FAKE, _sample(), ob, pv, None, pr, idx, prob), "null t_w"),
             ((FAKE, _sample(steps=0), ob, pv, tw, None, None, None), "steps"),
             ((FAKE, _sample(steps=51), ob, pv, tw, None, None, None), "steps"),
             ((FAKE, _sample(steps=-3), ob, pv, tw, None, None, None), "steps"),
             ((FAKE, _sample(start_mode=1), ob, pv, tw, None, None, None), "start_mode"),   # RD_REPLAY_START_COMMON
             ((FAKE, _sample(start_mode=2), ob, pv, tw, None, None, None), "start_mode"),
             ((FAKE, _sample(windows=0), ob, pv, tw, None, None, None), "windows"),
             ((FAKE, _sample(windows=-2), ob, pv, tw, None, None, None), "windows"),
             ((FAKE, _sample(window_base=-1), ob, pv, tw, None, None, None), "window_base"),
             ((FAKE, _sample(recent=-1), ob, pv, tw, None, None, None), "recent"),
             ((h, _sample(), ob, pv, tw, pr, idx, prob), "not enabled")]
    for args, word in cases:
        assert fn(*args) == RD_EINVAL, word
        assert "rd_replay_prio_sample_windows:" in _msg(lib) and word in _msg(lib), (word, _msg(lib))
    del raw, mem


def test_sample_rows_rejects_bad_arguments_before_any_device_call(lib):
    raw, (x, t, idx, prob, *_r) = _buffers()
    mem, h = _zero_handle()
    fn = lib.rd_replay_prio_sample_rows
    odd = ctypes.c_void_p(x.value + 4)
    cases = [((None, _sample(), x, t, idx, prob), "null handle"), ((FAKE, None, x, t, idx, prob), "null sample"),
             ((FAKE, _sample(), None, t, idx, prob), "null x"), ((FAKE, _sample(), x, None, idx, prob), "null t_pdflat"),
             ((FAKE, _sample(), odd, t, None, None), "aligned"), ((FAKE, _sample(windows=0), x, t, None, None), "windows"),
             ((FAKE, _sample(window_base=-5), x, t, None, None), "window_base"),
             ((FAKE, _sample(recent=-1), x, t, None, None), "recent"),
             ((h, _sample(), x, t, idx, prob), "not enabled")]
    for args, word in cases:
        assert fn(*args) == RD_EINVAL, word
        assert "rd_replay_prio_sample_rows:" in _msg(lib) and word in _msg(lib), (word, _msg(lib))
    del raw, mem


def test_drivers_take_replay_priority_keyword_only_default_none():
    from reacherdistilation_amd import lstm_train, mlp_train
    for mod in (lstm_train, mlp_train):
        p = inspect.signature(mod.train_envs).parameters["replay_priority"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "none", mod.__name__
        for value in ("record", "refresh", "bogus"):      # needs a ring / a known value: before any device call
            with pytest.raises(ValueError):
                mod.train_envs(4, 2, replay_priority=value, device="cuda:0")


# -- the model against itself -----------------------------------------------------------------
SEED = 0x0123_4567_89AB_CDEF


def _wrapped(cap=12, pushed=19, seed=SEED, **kw):
    """a ring after wrap: `pushed` random episodes through `cap` slots, random priorities"""
    rng = np.random.RandomState(3)
    m = PrioRingModel(cap, seed, **kw)
    for lo in range(0, pushed, cap):
        m.push_episodes(rng.standard_normal((min(cap, pushed - lo), STEPS, REC)).astype(np.float32))
    m.q[:] = rng.randint(1, 2 ** 24 + 1, m.q.shape)
    return m


@pytest.mark.parametrize("T", [1, 10, 50])
@pytest.mark.parametrize("recent", [0, 3])
def test_model_draw_ranges(T, recent):
    """ranks < count, starts <= 50 - T, only eligible slots, gathers from the drawn windows."""
    m = _wrapped()
    m.draws = 5
    B = 2048
    slot, start, prob = m.draw_prio(T, B, recent=recent, window_base=2 ** 33 + 5)
    count = min(12, recent) if recent else 12
    elig = m.eligible(recent)
    assert elig == [(19 - count + j) % 12 for j in range(count)] and len(elig) == count
    assert set(slot.tolist()) <= set(elig)
    rank = np.array([elig.index(s) for s in slot])
    assert rank.max() < count and start.min() >= 0 and start.max() <= 50 - T
    assert prob.dtype == np.float32 and (prob > 0).all() and (prob <= 1).all()
    W = m.window_weights(T, recent)
    total = sum(map(sum, W))
    assert np.array_equal(prob, np.array([np.float32(W[r][s] / total) for r, s in zip(rank, start)]))
    # the draw index, the window base and the table all move the stream; the uniform stream is another
    assert (m.draw_prio(T, B, recent=recent)[1] != start).any() or T == 50
    if T < 50:
        assert (m.draw(B, 51 - T, recent=recent, window_base=2 ** 33 + 5)[1] != start).any()
    out = m.sample_windows_prio(T, 64, recent=recent, window_base=2 ** 33 + 5)
    assert m.draws == 6 and out[4].dtype == np.int32 and np.array_equal(out[4][:, 0], slot[:64])
    for b in range(64):
        s0, st = out[4][b]
        assert np.array_equal(out[0][:, b], m.ring[s0, st:st + T, :11])
        assert np.array_equal(out[2][:, b], m.ring[s0, st:st + T, 12:16])


def test_model_rows_are_windows_of_one():
    m = _wrapped()
    a = m.sample_rows_prio(300, window_base=7)
    m.draws -= 1
    b = m.sample_windows_prio(1, 300, window_base=7)
    assert np.array_equal(a[2], b[4]) and np.array_equal(a[3], b[5])
    assert np.array_equal(a[0][:, :11], b[0][0]) and np.array_equal(a[0][:, 11:15], b[1][0])
    assert np.array_equal(a[0][:, 15:], b[3][0]) and np.array_equal(a[1], b[2][0])


def _counts(m, T, B, recent=0):
    slot, start, _ = m.draw_prio(T, B, recent=recent)
    c = np.zeros((m.capacity, STEPS + 1 - T), np.int64)
    np.add.at(c, (slot, start), 1)
    return c


@pytest.mark.parametrize("T", [1, 10, 50])
def test_a_table_of_ones_reproduces_the_uniform_law(T):
    """every eligible window has weight T: each (episode, start) has probability 1 / (count (51 - T)),
    and the reported prob says so exactly"""
    m = _wrapped(cap=8, pushed=8)
    m.fill(1)
    m.draws = 5
    B, n = 2 ** 16, 8 * (51 - T)
    slot, start, prob = m.draw_prio(T, B)
    assert (prob == np.float32(1.0 / n)).all()
    c = _counts(m, T, B)
    p = 1.0 / n
    assert np.abs(c - B * p).max() <= 5 * np.sqrt(B * p * (1 - p))
    # raw entries 0 read as 1 (the clamp): the same draw
    m.q[:] = 0
    s2, st2, _ = m.draw_prio(T, B)
    assert np.array_equal(s2, slot) and np.array_equal(st2, start)
    assert clamp(np.array([0, 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1], np.uint32)).tolist() == \
        [1, 1, 2 ** 24, 2 ** 24, 2 ** 24, 2 ** 24]


@pytest.mark.parametrize("T", [1, 10, 50])
def test_one_heavy_episode_takes_all_but_a_computable_share(T):
    m = _wrapped(cap=8, pushed=8)
    m.fill(1)
    m.q[3] = 2 ** 24
    m.draws = 5
    B = 2 ** 14
    slot, _, _ = m.draw_prio(T, B)
    light = 7 * T * (51 - T)                               # the seven other episodes' total weight
    share = light / (light + 2 ** 24 * T * (51 - T))       # = 7 / (7 + 2^24), 4.2e-7
    assert abs(share - 7 / (7 + 2 ** 24)) < 1e-18
    others = int((slot != 3).sum())
    assert others <= 1 + 5 * np.sqrt(B * share) + B * share, (others, B * share)   # 0 or 1 in 16,384 draws
    assert others < 3


@pytest.mark.parametrize("T", [1, 10, 50])
def test_frequencies_follow_the_weights(T):
    """8 stored episodes, random priorities with one episode at 2^24 and one at 1; B = 2^18 draws: every
    window whose expected count is >= 50 has its observed count within 5 sqrt(B p (1 - p)) of B p (this
    model's largest deviations are 2.80, 3.22 and 1.55 standard deviations at T = 1, 10, 50; a wrong
    prefix or an off-by-one start breaks the bound by orders of magnitude)."""
    m = PrioRingModel(8, SEED)
    m.pushed = 8
    m.q[:] = np.random.RandomState(7).randint(1, 2 ** 24 + 1, (8, 50))
    m.q[3], m.q[5] = 2 ** 24, 1
    m.draws = 5
    B = 2 ** 18
    c = _counts(m, T, B)
    W = np.array(m.window_weights(T), np.float64)
    slots = m.eligible()
    p = np.zeros_like(c, np.float64)
    p[slots] = W / W.sum()
    big = B * p >= 50
    assert big.sum() >= (51 - T) * 6 and c.sum() == B
    dev = np.abs(c - B * p) / np.sqrt(B * p * (1 - p) + 1e-300)
    print(f"T={T}: largest deviation {dev[big].max():.2f} standard deviations over {int(big.sum())} windows")
    assert dev[big].max() <= 5.0


def test_model_quantisation_and_pushes():
    t = np.zeros((6, 4), np.float32)
    S = np.array([[3, 4, 9, 9], [np.nan, 0, 0, 0], [np.inf, 0, 0, 0], [-np.inf, 1, 0, 0], [1e6, 1e6, 0, 0],
                  [1e-9, 0, 0, 0]], np.float32)
    assert quantise(S, t, SQERR, 0, 1).tolist() == [25, 2 ** 24, 2 ** 24, 2 ** 24, 2 ** 24, 1]
    assert quantise(S, t, ERR, 0, 7).tolist() == [7, 2 ** 24, 2 ** 24, 2 ** 24, 1414213, 7]
    assert quantise(S[:5], t[:5], ERR, 24, 1).tolist() == [2 ** 24] * 5
    assert quantise(S[5:], t[5:], ERR, 24, 1).tolist() == [1]                # 1e-9 x 2^24 truncates to 0: the floor
    assert quantise(np.float32([[0.5, 0]]), t[:1], ERR, 24, 1).tolist() == [2 ** 23]
    assert quantise(np.float32([[0.5, 0]]), t[:1], SQERR, 24, 1).tolist() == [2 ** 22]
    assert quantise(S, S, SQERR, 16, 1)[[0, 4, 5]].tolist() == [1, 1, 1]   # inf - inf and nan - nan stay at 2^24
    # pushes: INIT_RECORD scores the record's own s_pdflat against its t_pdflat; INIT_CONST writes q_init
    rng = np.random.RandomState(1)
    m = PrioRingModel(5, 0, measure=ERR, shift=16, q_min=3, q_init=77, init=INIT_RECORD)
    eps = rng.standard_normal((7, STEPS, REC)).astype(np.float32)
    m.push_episodes(eps[:4])
    assert np.array_equal(m.q[:4], quantise(eps[:4, :, 16:20], eps[:4, :, 12:16], ERR, 16, 3)) and (m.q[4] == 77).all()
    m.init = INIT_CONST
    m.q_init = 9
    m.push_episodes(eps[4:])                 # slots 4, 0, 1
    assert (m.q[[4, 0, 1]] == 9).all() and np.array_equal(m.q[2], quantise(eps[2, :, 16:20], eps[2, :, 12:16], ERR, 16, 3))


def test_model_update_takes_the_maximum_and_skips_bad_indices():
    m = _wrapped()
    before = m.q.copy()
    idx = np.array([[2, 7], [2, 7], [2, 7], [-1, 0], [12, 0], [3, -1], [4, 50], [5, 49]], np.int32)
    s = np.zeros((8, 4), np.float32)
    s[:, :2] = m.ring[2, 7, 12:14] + np.array([[0.5, 0], [2.0, 0], [1.0, 0], [9, 9], [9, 9], [9, 9], [9, 9], [0, 0]])
    s[7, :2] = m.ring[5, 49, 12:14] + np.float32(0.25)
    m.update(idx, s)
    changed = np.argwhere(m.q != before).tolist()
    assert sorted(changed) == [[2, 7], [5, 49]]
    three = [int(quantise(s[b], m.ring[2, 7, 12:16], SQERR, 16, 1)) for b in range(3)]
    assert three[1] > three[2] > three[0] and abs(three[1] - 4 * 2 ** 16) <= 1   # errors 0.5, 2, 1: the 2 wins
    assert m.q[2, 7] == three[1]
    assert m.q[5, 49] == quantise(s[7], m.ring[5, 49, 12:16], SQERR, 16, 1)
    # windows: start 45 with T = 10 is skipped; overlapping windows share records
    before = m.q.copy()
    idxw = np.array([[6, 45], [6, 0], [6, 5], [12, 0]], np.int32)
    sw = np.random.RandomState(5).standard_normal((10, 4, 4)).astype(np.float32)
    m.update(idxw, sw)
    assert (m.q[6, 15:] == before[6, 15:]).all() and (np.delete(m.q, 6, 0) == np.delete(before, 6, 0)).all()
    for rec in range(5, 10):                                # named by window 1 (p = rec) and window 2 (p = rec - 5)
        a = quantise(sw[rec, 1], m.ring[6, rec, 12:16], SQERR, 16, 1)
        b = quantise(sw[rec - 5, 2], m.ring[6, rec, 12:16], SQERR, 16, 1)
        assert m.q[6, rec] == max(a, b)
