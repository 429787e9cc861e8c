"""Host-side (no GPU) checks of the replay ring's ABI (include/reacher_replay.h): every declared
rd_replay_* name is exported, the ctypes mirrors match the header field by field, every argument check
that needs no handle answers before any device call and before the handle is read, and the NumPy model
the GPU tests compare against (tests/replay_model.py) is consistent with itself.  The checks that read
the handle (windows > max_batch, a ring never pushed to, the capacity rule of the pushes) are in
tests/test_replay_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.replay_model import REC, START_COMMON, STEPS, RingModel

HEADER = "reacher_replay.h"
RD_EINVAL = -100000


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, replay  # noqa: F401  (replay registers the symbols)
    build.build(verbose=False)
    return _native.load()


def _header():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _c_layout(struct, fields):
    """sizeof and offsetof of the header's struct, compiled with gcc from the header itself."""
    body = "\n".join(f'printf("{f} %zu\\n", offsetof({struct}, {f}));' for f in fields)
    src = (f'#include <stddef.h>\n#include <stdio.h>\n#include "{HEADER}"\n'
           f'int main(void) {{ printf("sizeof %zu\\n", sizeof({struct})); {body} return 0; }}\n')
    d = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(d, exist_ok=True)
    c, exe = os.path.join(d, f"layout_{struct}.c"), os.path.join(d, f"layout_{struct}")
    with open(c, "w") as fh:
        fh.write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in res.splitlines())}


def test_every_declared_name_is_exported_with_a_signature(lib):
    from reacherdistilation_amd import _native
    names = sorted(set(re.findall(r"\b(rd_replay_[a-z0-9_]+)\s*\(", _header())))
    assert names == sorted(["rd_replay_create", "rd_replay_destroy", "rd_replay_set_stream", "rd_replay_reset",
                            "rd_replay_ring", "rd_replay_counters", "rd_replay_push_steps", "rd_replay_push_episodes",
                            "rd_replay_push_rows", "rd_replay_sample_windows", "rd_replay_sample_rows"])
    have = _native.exported_symbols()
    for name in names:
        assert have.get(name) is True, name
        assert getattr(lib, name).argtypes is not None, name


@pytest.mark.parametrize("cls,struct,size", [("RdReplayConfig", "rd_replay_config", 16),
                                             ("RdReplaySample", "rd_replay_sample", 40)])
def test_ctypes_mirrors_match_the_header(cls, struct, size):
    from reacherdistilation_amd import replay
    C = getattr(replay, cls)
    fields = [f[0] for f in C._fields_]
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct + ";", _header()).group(1)
    assert fields == re.findall(r"(\w+)\s*(?:,|;)", body)   # same members, same order
    c = _c_layout(struct, fields)
    assert c["sizeof"] == ctypes.sizeof(C) == size
    for f in fields:
        assert c[f] == getattr(C, f).offset, f


def test_constants_match_the_header():
    from reacherdistilation_amd import replay
    txt = _header()
    for name, value in (("RD_REPLAY_START_PER_WINDOW", replay.START_PER_WINDOW),
                        ("RD_REPLAY_START_COMMON", replay.START_COMMON), ("RD_REPLAY_MAX_BATCH", replay.MAX_BATCH),
                        ("RD_REPLAY_EPISODE_STEPS", STEPS), ("RD_REPLAY_RECORD", REC)):
        assert re.search(rf"#define {name} {value}\b", txt), name
    assert replay.REC == REC and replay.ROW == 16


def _msg(lib):
    return lib.rd_last_error().decode()


FAKE = ctypes.c_void_p(0x1000)   # a non-NULL handle that a rejected call never dereferences


def _buffers(n=6):
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


def test_create_rejects_bad_arguments_before_any_device_call(lib):
    """No GPU here: an answer at all shows that the check precedes every HIP call."""
    from reacherdistilation_amd.replay import RdReplayConfig
    h = ctypes.c_void_p()
    good = RdReplayConfig(capacity=8, max_batch=8)
    assert lib.rd_replay_create(None, ctypes.byref(good), None, 0, None) == RD_EINVAL
    assert "rd_replay_create" in _msg(lib) and "null out" in _msg(lib)
    assert lib.rd_replay_create(ctypes.byref(h), None, None, 0, None) == RD_EINVAL
    assert "rd_replay_create" in _msg(lib) and "null config" in _msg(lib)
    for field, value in (("capacity", 0), ("capacity", -1), ("capacity", 2 ** 31), ("max_batch", 0),
                         ("max_batch", 2 ** 22 + 1)):
        cfg = RdReplayConfig(capacity=8, max_batch=8)
        setattr(cfg, field, value)
        assert lib.rd_replay_create(ctypes.byref(h), ctypes.byref(cfg), None, 0, None) == RD_EINVAL, (field, value)
        assert "rd_replay_create" in _msg(lib) and field in _msg(lib)
    assert not h.value


def test_handle_calls_reject_a_null_handle(lib):
    for fn, args in (("rd_replay_set_stream", (None, None)), ("rd_replay_reset", (None,)),
                     ("rd_replay_counters", (None, None, None))):
        assert getattr(lib, fn)(*args) == RD_EINVAL
        assert fn in _msg(lib) and "null handle" in _msg(lib)
    assert lib.rd_replay_ring(None) is None
    assert lib.rd_replay_destroy(None) == 0


def test_pushes_reject_bad_arguments_before_any_device_call(lib):
    raw, (rec, x, t, s, rew, carry) = _buffers()
    cases = [("rd_replay_push_steps", (None, rec, 50, 4), "null handle"),
             ("rd_replay_push_steps", (FAKE, None, 50, 4), "null records"),
             ("rd_replay_push_steps", (FAKE, rec, 0, 4), "steps"),
             ("rd_replay_push_steps", (FAKE, rec, 49, 4), "steps"),
             ("rd_replay_push_steps", (FAKE, rec, 75, 4), "steps"),
             ("rd_replay_push_steps", (FAKE, rec, -50, 4), "steps"),
             ("rd_replay_push_steps", (FAKE, rec, 50, 0), "n_envs"),
             ("rd_replay_push_episodes", (None, rec, 2), "null handle"),
             ("rd_replay_push_episodes", (FAKE, None, 2), "null records"),
             ("rd_replay_push_episodes", (FAKE, rec, 0), "episodes"),
             ("rd_replay_push_rows", (None, x, t, s, rew, carry, 50, 4, 1.0), "null handle"),
             ("rd_replay_push_rows", (FAKE, None, t, s, rew, carry, 50, 4, 1.0), "null x"),
             ("rd_replay_push_rows", (FAKE, x, None, s, rew, carry, 50, 4, 1.0), "null t_pdflat"),
             ("rd_replay_push_rows", (FAKE, x, t, None, None, None, 50, 4, 1.0), "null reward"),
             ("rd_replay_push_rows", (FAKE, x, t, None, rew, None, 30, 4, 1.0), "steps"),
             ("rd_replay_push_rows", (FAKE, x, t, None, rew, None, 50, -1, 1.0), "n_envs")]
    for fn, args, word in cases:
        assert getattr(lib, fn)(*args) == RD_EINVAL, (fn, word)
        assert fn + ":" in _msg(lib) and word in _msg(lib), (fn, word, _msg(lib))
    del raw


def test_sample_windows_rejects_bad_arguments_before_any_device_call(lib):
    raw, (ob, pv, tw, pr, idx, _) = _buffers()
    fn = lib.rd_replay_sample_windows
    cases = [((None, _sample(), ob, pv, tw, pr, idx), "null handle"),
             ((FAKE, None, ob, pv, tw, pr, idx), "null sample"),
             ((FAKE, _sample(), None, pv, tw, pr, idx), "null ob_w"),
             ((FAKE, _sample(), ob, None, tw, pr, idx), "null prev_w"),
             ((FAKE, _sample(), ob, pv, None, pr, idx), "null t_w"),
             ((FAKE, _sample(steps=0), ob, pv, tw, None, None), "steps"),
             ((FAKE, _sample(steps=51), ob, pv, tw, None, None), "steps"),
             ((FAKE, _sample(steps=-3), ob, pv, tw, None, None), "steps"),
             ((FAKE, _sample(windows=0), ob, pv, tw, None, None), "windows"),
             ((FAKE, _sample(windows=-2), ob, pv, tw, None, None), "windows"),
             ((FAKE, _sample(start_mode=2), ob, pv, tw, None, None), "start_mode"),
             ((FAKE, _sample(start_mode=-1), ob, pv, tw, None, None), "start_mode"),
             ((FAKE, _sample(window_base=-1), ob, pv, tw, None, None), "window_base"),
             ((FAKE, _sample(recent=-1), ob, pv, tw, None, None), "recent")]
    for args, word in cases:
        assert fn(*args) == RD_EINVAL, word
        assert "rd_replay_sample_windows:" in _msg(lib) and word in _msg(lib), (word, _msg(lib))
    del raw


def test_sample_rows_rejects_bad_arguments_before_any_device_call(lib):
    raw, (x, t, idx, *_rest) = _buffers()
    fn = lib.rd_replay_sample_rows
    odd = ctypes.c_void_p(x.value + 4)
    cases = [((None, _sample(), x, t, idx), "null handle"),
             ((FAKE, None, x, t, idx), "null sample"),
             ((FAKE, _sample(), None, t, idx), "null x"),
             ((FAKE, _sample(), x, None, idx), "null t_pdflat"),
             ((FAKE, _sample(), odd, t, None), "aligned"),
             ((FAKE, _sample(windows=0), x, t, None), "windows"),
             ((FAKE, _sample(window_base=-5), x, t, None), "window_base"),
             ((FAKE, _sample(recent=-1), x, t, None), "recent")]
    for args, word in cases:
        assert fn(*args) == RD_EINVAL, word
        assert "rd_replay_sample_rows:" in _msg(lib) and word in _msg(lib), (word, _msg(lib))
    del raw


def test_drivers_take_the_replay_arguments_with_defaults_off():
    import inspect
    from reacherdistilation_amd import lstm_train, mlp_train
    for mod in (lstm_train, mlp_train):
        sig = inspect.signature(mod.train_envs)
        for k, v in dict(replay_capacity=0, replay_windows=0, updates_per_act=1, replay_recent=0).items():
            p = sig.parameters[k]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == v, (mod.__name__, k)


# -- the model against itself -----------------------------------------------------------------
def _episodes(rng, E):
    return rng.standard_normal((E, STEPS, REC)).astype(np.float32)


def test_model_slots_after_wrap():
    rng = np.random.RandomState(0)
    m = RingModel(5)
    eps = _episodes(rng, 12)
    m.push_episodes(eps[:4])
    assert m.pushed == 4 and m.stored() == 4
    np.testing.assert_array_equal(m.ring[:4], eps[:4])
    m.push_episodes(eps[4:9])       # wraps: episodes 4..8 -> slots 4, 0, 1, 2, 3
    m.push_episodes(eps[9:12])      # episodes 9..11 -> slots 4, 0, 1
    assert m.pushed == 12 and m.stored() == 5
    for g in range(7, 12):          # the five newest, each in slot g % 5
        np.testing.assert_array_equal(m.ring[g % 5], eps[g])


def test_model_push_steps_and_rows_are_the_episode_form():
    rng = np.random.RandomState(1)
    K, n = 100, 3
    r = rng.standard_normal((K, n, REC)).astype(np.float32)
    a, b = RingModel(7), RingModel(7)
    a.push_steps(r)
    b.push_episodes(np.stack([r[blk * 50:(blk + 1) * 50, i] for blk in range(2) for i in range(n)]))
    np.testing.assert_array_equal(a.ring, b.ring)
    # rows: the record's rew is the previous step's reward, the carry at k = 0
    x = rng.standard_normal((K, n, 16)).astype(np.float32)
    t, s = rng.standard_normal((2, K, n, 4)).astype(np.float32)
    rew, carry = rng.standard_normal((K, n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    c = RingModel(7)
    c.push_rows(x, t, s, rew, carry, stepped_with=1.0)
    ep = c.ring[1 * n + 2]   # second block of 50 steps, env 2
    np.testing.assert_array_equal(ep[:, :11], x[50:, 2, :11])
    np.testing.assert_array_equal(ep[:, 11], rew[49:99, 2])
    np.testing.assert_array_equal(c.ring[2][0, 11], carry[2])
    np.testing.assert_array_equal(ep[:, 12:16], t[50:, 2])
    np.testing.assert_array_equal(ep[:, 16:20], s[50:, 2])
    assert (ep[:, 20] == 1.0).all()


@pytest.mark.parametrize("T", [1, 10, 50])
@pytest.mark.parametrize("pushed,recent", [(3, 0), (8, 0), (19, 0), (19, 3), (2, 3)])
def test_model_draw_ranges(T, pushed, recent):
    """ranks < count, starts <= 50 - T, `recent` honoured, slot arithmetic after wrap."""
    cap, B = 8, 4096
    m = RingModel(cap, seed=0x1234_5678_9ABC_DEF0)
    m.pushed, m.draws = pushed, 5
    slot, start = m.draw(B, 51 - T, recent=recent, window_base=2 ** 33 + 5)
    count = min(pushed, cap) if not recent else min(pushed, cap, recent)
    assert start.min() >= 0 and start.max() <= 50 - T
    if T < 50:
        assert len(set(start.tolist())) == 51 - T       # every start is reached at this B
    else:
        assert (start == 0).all()
    eligible = {g % cap for g in range(pushed - count, pushed)}   # the `count` newest episodes
    assert set(slot.tolist()) == eligible                # nothing outside, and all of them at this B
    rank = (slot - (pushed - count)) % cap
    assert rank.max() < count
    # a common start: one value for the batch, per-window episodes unchanged
    slot_c, start_c = m.draw(B, 51 - T, recent=recent, window_base=2 ** 33 + 5, common=True)
    np.testing.assert_array_equal(slot_c, slot)
    assert len(set(start_c.tolist())) == 1
    # the draw index and the window base both move the stream
    m.draws += 1
    assert (m.draw(B, 51 - T, recent=recent)[0] != slot).any() or count == 1
    # only the low 32 bits of `draws` enter
    m.draws = 5 + 2 ** 32
    np.testing.assert_array_equal(m.draw(B, 51 - T, recent=recent, window_base=2 ** 33 + 5)[0], slot)


def test_model_windows_follow_the_dataset_prev_rule():
    rng = np.random.RandomState(2)
    m = RingModel(6, seed=3)
    m.push_episodes(_episodes(rng, 6))
    m.push_episodes(_episodes(rng, 2))
    T, B = 10, 300
    ob_w, prev_w, t_w, prew_w, idx = m.sample_windows(T, B)
    assert m.draws == 1 and idx.dtype == np.int32
    for b in range(B):
        slot, start = idx[b]
        ep = m.ring[slot]
        np.testing.assert_array_equal(ob_w[:, b], ep[start:start + T, :11])
        np.testing.assert_array_equal(t_w[:, b], ep[start:start + T, 12:16])
        for p in range(T):
            j = start + p
            want = np.zeros(5, np.float32) if j == 0 else np.concatenate([ep[j - 1, 12:16], ep[j - 1, 11:12]])
            np.testing.assert_array_equal(np.concatenate([prev_w[p, b], prew_w[p, b]]), want)
    assert (idx[:, 1] == 0).any()   # the zero-prev branch was exercised
    # the common start is the batch's single start; the next sample uses the next draw index
    _, _, _, _, idx_c = m.sample_windows(T, B, start_mode=START_COMMON)
    assert m.draws == 2 and len(set(idx_c[:, 1].tolist())) == 1
    x, t, idx_r = m.sample_rows(B)
    for b in range(B):
        slot, s = idx_r[b]
        ep = m.ring[slot]
        prev = np.zeros(5, np.float32) if s == 0 else np.concatenate([ep[s - 1, 12:16], ep[s - 1, 11:12]])
        np.testing.assert_array_equal(x[b], np.concatenate([ep[s, :11], prev]))
        np.testing.assert_array_equal(t[b], ep[s, 12:16])
