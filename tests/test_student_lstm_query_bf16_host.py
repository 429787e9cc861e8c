"""Host-side checks of the LSTM student's bf16 closed-loop query (rdl_set_query_dtype,
StudentLstmConfig.query_dtype): the library, the header and the ctypes layer carry the two calls; a
bad query dtype raises before any native call; and the emulation chain that
tests/test_student_lstm_query_bf16_gpu.py compares the records against (tests/lstm_query_bf16.py)
is the f64 oracle chain when nothing is rounded, with bounds an f32 device can meet.

Measured here (17 envs x 100 queries on synthetic records, T = 10; forward_f32 is the stand-in with f32
sums): median |stand-in - emulation| 1.3e-5, max 1.4e-4, against the cap max |emulation - oracle|
7.3e-4.  A single forward's stand-in differs by 4e-8 / 4.4e-5 (tests/test_student_lstm_bf16_gpu.py): over
the chain a rounding that flips near a tie stays in the carried state, in both restatements.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import lstm_bf16 as lb
from tests import lstm_query_bf16 as lq


def _records(E=2, n=17, seed=4):
    """Synthetic records [E, n, 50, 21]: the fields a query's window reads, ob and t_pdflat, in the
    ranges of tests/lstm_bf16.batch; the rest zero."""
    rs = np.random.RandomState(seed)
    rec = np.zeros((E, n, lq.STEPS, 21), np.float32)
    rec[..., :lq.F_REW] = rs.uniform(-1, 1, (E, n, lq.STEPS, 11))
    rec[..., lq.F_T:lq.F_T + 2] = rs.uniform(-.5, .5, (E, n, lq.STEPS, 2))
    rec[..., lq.F_T + 2:lq.F_S] = rs.uniform(-1, 0, (E, n, lq.STEPS, 2))
    return rec


def test_unrounded_emulation_chain_is_the_oracle_chain():
    from tests.test_student_lstm_evaluate_gpu import _oracle_chain
    rec, p = _records(), lb.params()
    got, want = lq.emulation_chain(rec, p, 10, rounded=False), _oracle_chain(rec, p, 10)
    assert got.shape == (2, 17, 50, 4) and np.abs(want).max() > 1e-2
    assert np.abs(got - want).max() <= 1e-12


def test_an_f32_stand_in_of_the_rounded_chain_stays_inside_the_gpu_tests_bounds():
    """The bounds of the GPU test's third check are reachable: an f32-sum restatement of the device's
    arithmetic, fed the same records, with its own state chained over the 100 queries."""
    rec, p = _records(), lb.params()
    emu = lq.emulation_chain(rec, p, 10)
    ora = lq.emulation_chain(rec, p, 10, rounded=False)
    got = lq.emulation_chain(rec, p, 10, forward=lq.forward_f32)
    med, mx, cap = lq.bounds(got, emu, ora)
    print(f"median |stand-in - emulation| {med:.3e}  max {mx:.3e}  cap max |emulation - oracle| {cap:.3e}")
    assert med <= 5e-5, med
    assert mx <= cap, (mx, cap)
    assert cap > 2e-5   # bf16's error is there to bound with
    # and the stand-in of the UNROUNDED chain is not inside them: the bounds tell the two arithmetics apart
    f32 = lq.emulation_chain(rec, p, 10, rounded=False, forward=lq.forward_f32)
    assert lq.bounds(f32, emu, ora)[1] > 0.5 * cap


def test_the_library_exports_the_two_calls_and_the_header_declares_them():
    """No GPU here: the setter is host-only, so its answers to bad arguments show through rd_last_error."""
    from reacherdistilation_amd import _native, build
    from tests.conftest import ROOT
    build.build(verbose=False)
    lib = _native.load()
    assert lib.rdl_query_dtype(None) == -1
    assert lib.rdl_set_query_dtype(None, 0) == -100000
    msg = lib.rd_last_error().decode()
    assert "rdl_set_query_dtype" in msg and "null" in msg
    txt = open(os.path.join(ROOT, "include", "reacher_student_lstm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int rdl_set_query_dtype\(rdl_trainer\* t, int32_t dtype\);", code)
    assert re.search(r"int rdl_query_dtype\(const rdl_trainer\* t\);", code)
    assert "Which calls stay f32" not in txt and "rdl_set_query_dtype" in txt.split("#ifndef")[0]


@pytest.mark.parametrize("kw", [dict(dtype="f32", query_dtype="bf16"), dict(query_dtype="bf16"),
                                dict(dtype="bf16", query_dtype="fp16"), dict(query_dtype=""), dict(query_dtype=None),
                                dict(dtype="bf16", query_dtype=1)])
def test_a_bad_query_dtype_raises_before_any_native_call(kw, monkeypatch):
    from reacherdistilation_amd import _native, student_lstm

    def no_native(*a, **k):
        raise AssertionError("native layer reached")
    monkeypatch.setattr(_native, "load", no_native)
    with pytest.raises(ValueError, match="query_dtype"):
        student_lstm.StudentLstmConfig(**kw)
    cfg = student_lstm.StudentLstmConfig(dtype=kw.get("dtype", "f32"))
    cfg.query_dtype = kw["query_dtype"]   # set after construction: still caught, before the library is loaded
    with pytest.raises(ValueError, match="query_dtype"):
        student_lstm.StudentLstmTrainer(cfg, device="cuda:0")


def test_config_and_drivers_carry_the_query_dtype():
    from reacherdistilation_amd import evaluate, lstm_train, student_lstm
    cfg = student_lstm.StudentLstmConfig
    assert cfg().query_dtype == "f32" and cfg().native_query_dtype() == 0
    assert cfg(dtype="bf16").query_dtype == "f32"   # an opt-in: a bf16 trainer's query stays f32 by default
    assert cfg(dtype="bf16", query_dtype="bf16").native_query_dtype() == 1
    assert ctypes.sizeof(student_lstm.RdlConfig) == 64   # the struct did not grow: the setting has its own call
    for fn in (lstm_train.train_envs, evaluate.evaluate_student_lstm):
        assert inspect.signature(fn).parameters["query_dtype"].default == "f32"
    for name in ("set_query_dtype", "query_dtype"):
        assert hasattr(student_lstm.StudentLstmTrainer, name)
