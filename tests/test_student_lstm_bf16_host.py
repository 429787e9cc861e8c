"""Host-side checks of the LSTM student's bf16 mode (rdl_create_dtype, StudentLstmConfig.dtype): the
emulation tests/lstm_bf16.py that the GPU tests compare against is the f64 oracle when nothing is
rounded and differs from it by bf16's error when the cell matrix's products are; the header, the
ctypes layer and the library carry the create call, with rdl_config's layout as it was; a bad dtype
raises before any native call.

Measured (tests/lstm_bf16.params, .batch; the shapes of tests/test_student_lstm_bf16_gpu.py): the
rounded emulation against the f64 oracle: pdflat max 3.6e-4 .. 6.9e-4, 68-75 % of the outputs outside
5e-5 + 1e-4 |ref|, gradient relative L2 3.4e-4 .. 1.7e-3.  bf16 has 8 significand bits (unit roundoff
2^-9 = 2e-3); the sums over 243 and 800 products average it down.  The bounds below bracket those.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle import lstm_np as ln
from tests import lstm_bf16 as lb


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("T,B,with_state", [(10, 20, False), (3, 130, True)])
def test_unrounded_emulation_is_the_oracle(loss, T, B, with_state):
    p = lb.params(T=T)
    ob, prev, t = lb.batch(T, B, B)
    st = lb.state(B) if with_state else None
    fw, want = lb.forward(p, ob, prev, st, rounded=False), ln.forward(p, ob, prev, st)
    np.testing.assert_array_equal(fw["pdflat"], want["pdflat"])
    np.testing.assert_array_equal(np.stack(fw["state"]), np.stack(want["state"]))
    _, d, _ = ln.loss_and_dout(want["pdflat"], t, loss, T * B)
    assert lb.rel_l2(lb.backward(p, fw, d, rounded=False), ln.backward(p, want, d)) <= 1e-15
    g, lval, sq, _ = lb.step_gradient(p, ob, prev, t, loss, st, rounded=False)
    L, _, s = ln.loss_and_dout(want["pdflat"], t, loss, T * B)
    assert lb.rel_l2(g, ln.backward(p, want, d)) <= 1e-15 and lval == L and sq == s


@pytest.mark.parametrize("T,B", [(10, 20), (3, 130)])
def test_rounded_products_differ_by_bf16s_error(T, B):
    p = lb.params(T=T)
    ob, prev, t = lb.batch(T, B, B)
    got, want = lb.forward(p, ob, prev)["pdflat"], ln.forward(p, ob, prev)["pdflat"]
    err = np.abs(got - want)
    assert 2e-5 < np.median(err) and err.max() < 5e-3, (np.median(err), err.max())
    assert lb.outside(got, want) >= 0.5
    for loss in ("mse", "kl"):
        g, _, _, _ = lb.step_gradient(p, ob, prev, t, loss)
        gw, _, _, _ = lb.step_gradient(p, ob, prev, t, loss, rounded=False)
        assert 2e-4 < lb.rel_l2(g, gw) < 2e-2, lb.rel_l2(g, gw)


def test_only_the_cell_matrix_products_are_rounded():
    """With Wl and its operands exactly representable in bf16 the rounded emulation is the oracle:
    nothing else rounds.  (x is not representable in general, so zero the x rows of Wl and start
    from h = 0 with T = 1: the gate product is then exactly bl.)"""
    T, B = 1, 7
    p = lb.params(T=T)
    o, s = ln.layout(T)[0]["Wl"]
    p[o:o + s[0] * s[1]] = 0.0
    ob, prev, t = lb.batch(T, B, 3)
    fw, want = lb.forward(p, ob, prev), ln.forward(p, ob, prev)
    np.testing.assert_array_equal(fw["pdflat"], want["pdflat"])
    _, d, _ = ln.loss_and_dout(want["pdflat"], t, "kl", T * B)
    g, gw = lb.backward(p, fw, d), ln.backward(p, want, d)
    lay = ln.layout(T)[0]
    for k in ("bl",) + tuple(f"h0/{n}" for n in ("W1", "b1", "W5", "b5")):   # dbl sums the unrounded dz
        o, s = lay[k]
        np.testing.assert_array_equal(g[o:o + int(np.prod(s))], gw[o:o + int(np.prod(s))])


def test_config_carries_the_dtype():
    from reacherdistilation_amd.student_lstm import DTYPES, RdlConfig, StudentLstmConfig
    assert DTYPES == {"f32": 0, "bf16": 1}
    assert StudentLstmConfig().dtype == "f32" and StudentLstmConfig().native_dtype() == 0
    assert StudentLstmConfig(dtype="bf16", loss="mse").native_dtype() == 1
    # the struct did not grow: the dtype travels beside it
    assert [f[0] for f in RdlConfig._fields_] == ["loss", "lr", "beta1", "beta2", "eps", "steps", "max_windows",
                                                  "metrics_len", "keep_prob", "seed", "row_base", "kernels"]
    assert ctypes.sizeof(RdlConfig) == 64 and RdlConfig.kernels.offset == 56


def test_header_defines_the_dtypes_and_states_the_arithmetic():
    from tests.conftest import ROOT
    txt = open(os.path.join(ROOT, "include", "reacher_student_lstm.h")).read()
    assert re.search(r"#define RDL_DTYPE_F32 0\b", txt) and re.search(r"#define RDL_DTYPE_BF16 1\b", txt)
    assert re.search(r"^ \* Arithmetic\.", txt, re.M)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int rdl_create_dtype\(rdl_trainer\*\* out, const rdl_config\* cfg, int32_t dtype, int device, "
                     r"void\* hip_stream\);", code)


def test_the_library_exports_the_create_call_and_refuses_bad_arguments():
    """No GPU here: an answer at all shows that the checks precede every HIP call."""
    from reacherdistilation_amd import _native, build, student_lstm
    build.build(verbose=False)
    lib = _native.load()
    c = student_lstm.RdlConfig(loss=1, lr=1e-3, beta1=.9, beta2=.999, eps=1e-8, steps=10, max_windows=20,
                               metrics_len=0, keep_prob=1.0, seed=0, row_base=0, kernels=0)
    h = ctypes.c_void_p()
    assert lib.rdl_create_dtype(None, ctypes.byref(c), 1, 0, None) == -100000
    assert lib.rdl_create_dtype(ctypes.byref(h), None, 1, 0, None) == -100000 and not h.value
    for bad in (2, -1, 7):
        assert lib.rdl_create_dtype(ctypes.byref(h), ctypes.byref(c), bad, 0, None) == -100000 and not h.value


@pytest.mark.parametrize("bad", ["fp16", "BF16", "", None, 1])
def test_a_bad_dtype_raises_before_any_native_call(bad, monkeypatch):
    from reacherdistilation_amd import _native, student_lstm

    def no_native(*a, **k):
        raise AssertionError("native layer reached")
    monkeypatch.setattr(_native, "load", no_native)
    with pytest.raises(ValueError, match="dtype"):
        student_lstm.StudentLstmConfig(dtype=bad)
    cfg = student_lstm.StudentLstmConfig()
    cfg.dtype = bad   # set after construction: still caught, before the library is loaded
    with pytest.raises(ValueError, match="dtype"):
        student_lstm.StudentLstmTrainer(cfg, device="cuda:0")


def test_the_drivers_take_the_dtype():
    from reacherdistilation_amd import lstm_train
    for fn in (lstm_train.train, lstm_train.train_envs, lstm_train.train_bptt):
        assert inspect.signature(fn).parameters["dtype"].default == "f32"
