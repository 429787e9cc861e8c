"""Host-side checks of the reference MLP student's bf16 mode (rdm_create_dtype, StudentMlpConfig.dtype):
the emulation tests/refnet_bf16.py that the GPU tests compare against is the f64 oracle when no layer
is rounded and differs from it by bf16's error when layers 1-3 are; the config carries the mode to
the create call, with rdm_config's layout as it was; a bad string raises before any native call.

Measured (Glorot seed 2, biases U(+-0.2), refnet_bf16.batch rows, n = 64 .. 4,099): bf16 definition
against the f64 oracle: forward median 1.0e-3, max 5.4e-3 .. 6.8e-3, 97-100 % of the outputs outside
2e-5 + 1e-4 |ref|, gradient relative L2 2.5e-3 .. 4.6e-3.  An f32-accumulating stand-in for the
kernel against the f64-accumulating emulation: forward median 1.5e-8, at most 0.18 % outside,
gradient relative L2 <= 1.3e-5.  The bounds below bracket those figures: bf16 has 8 significand
bits (unit roundoff 2^-9 = 2e-3), f32 sums 2^-24.
"""
import ctypes

import numpy as np
import pytest

from oracle import policy_np as pn
from oracle import refnet_np as rn
from tests import refnet_bf16 as rb

SIZES = [64, 200, 4099]


@pytest.mark.parametrize("loss", ["mse", "kl"])
def test_unrounded_emulation_is_the_oracle(loss):
    p = rb.params()
    x, t = rb.batch(200, 1)
    fw, want = rb.forward(p, x, rounded=()), rn.forward(p, x)
    for a, b in zip(fw["hs"], want["hs"]):
        np.testing.assert_array_equal(a, b)
    _, d, _ = rn.loss_and_dout(want["pdflat"], t, loss, 200)
    np.testing.assert_array_equal(rb.backward(p, fw, d, rounded=()), rn.backward(p, want, d))


@pytest.mark.parametrize("n", SIZES)
def test_rounded_layers_differ_by_bf16s_error(n):
    p = rb.params()
    x, t = rb.batch(n, n)
    got, want = rb.forward(p, x)["pdflat"], rn.forward(p, x)["pdflat"]
    err = np.abs(got - want)
    assert 2e-4 < np.median(err) < 4e-3 and err.max() < 3e-2, (np.median(err), err.max())
    assert rb.outside(got, want) >= 0.9
    for loss in ("mse", "kl"):
        g, _, _ = rb.step_gradient(p, x, t, loss)
        gw, _, _ = rb.step_gradient(p, x, t, loss, rounded=())
        assert 1e-3 < rb.rel_l2(g, gw) < 2e-2, rb.rel_l2(g, gw)
        # db sums the unrounded dZ: the last layer's bias gradient sees bf16 only through the forward
        assert np.abs(g[-4:] - gw[-4:]).max() <= 3e-2 * np.abs(gw[-4:]).max()


def test_only_layers_1_to_3_are_rounded():
    """Layer 0 sees the raw inputs and layer 4 emits the mean and log-std: both exact."""
    p = rb.params()
    x, _ = rb.batch(64, 3)
    fw, want = rb.forward(p, x), rn.forward(p, x)
    np.testing.assert_array_equal(fw["hs"][1], want["hs"][1])
    W4, b4 = rn.unpack(p.astype(np.float64))[4]
    np.testing.assert_array_equal(fw["pdflat"], fw["hs"][4] @ W4 + b4)
    assert rb.BF_LAYERS == (1, 2, 3)


def _forward_f32_sums(p, x):
    """A stand-in for the kernel: the same roundings, activations and sums in f32."""
    h = np.asarray(x, np.float32)
    for li, ((W, b), act) in enumerate(zip(rn.unpack(np.asarray(p, np.float32)), rn.ACT)):
        on = li in rb.BF_LAYERS
        a, w = (pn.bf16(h).astype(np.float32), pn.bf16(W).astype(np.float32)) if on else (h, W)
        z = (a @ w + b).astype(np.float32)
        h = np.tanh(z).astype(np.float32) if act else z
    return h


@pytest.mark.parametrize("n", SIZES)
def test_f32_sums_stay_inside_the_gpu_tests_caps(n):
    """The caps of tests/test_student_mlp_bf16_gpu.py leave room for f32 sums and the few bf16
    rounding flips they cause: the definition alone is well inside them."""
    p = rb.params()
    x, _ = rb.batch(n, n)
    got, want = _forward_f32_sums(p, x).astype(np.float64), rb.forward(p, x)["pdflat"]
    assert rb.outside(got, want) <= 0.01 and np.median(np.abs(got - want)) <= 2e-5


def test_config_carries_the_dtype():
    from reacherdistilation_amd.student_mlp import DTYPES, RdmConfig, StudentMlpConfig
    assert DTYPES == {"f32": 0, "bf16": 1}
    assert StudentMlpConfig().dtype == "f32" and StudentMlpConfig().native()[1] == 0
    c, dtype = StudentMlpConfig(dtype="bf16", loss="mse", keep_prob=0.5, seed=7).native(row_base=12)
    assert isinstance(c, RdmConfig) and dtype == 1 and c.loss == 0 and c.row_base == 12 and c.seed == 7
    assert ctypes.sizeof(RdmConfig) == 48 and RdmConfig._fields_[-1][0] == "row_base"   # the struct did not grow


def test_header_defines_the_dtypes():
    import os
    import re

    from tests.conftest import ROOT
    txt = open(os.path.join(ROOT, "include", "reacher_student_mlp.h")).read()
    assert re.search(r"#define RDM_DTYPE_F32 0\b", txt) and re.search(r"#define RDM_DTYPE_BF16 1\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int rdm_create_dtype\(rdm_trainer\*\* out, const rdm_config\* cfg, int32_t dtype, int device, "
                     r"void\* hip_stream\);", code)


def test_the_library_exports_the_create_call_and_refuses_null_arguments():
    """No GPU here: an answer at all shows that the check precedes every HIP call."""
    from reacherdistilation_amd import _native, build, student_mlp
    build.build(verbose=False)
    lib = _native.load()
    c, dtype = student_mlp.StudentMlpConfig(dtype="bf16").native()
    assert lib.rdm_create_dtype(None, ctypes.byref(c), dtype, 0, None) == -100000
    h = ctypes.c_void_p()
    assert lib.rdm_create_dtype(ctypes.byref(h), None, dtype, 0, None) == -100000 and not h.value


@pytest.mark.parametrize("bad", ["fp16", "BF16", "", None, 1])
def test_a_bad_dtype_raises_before_any_native_call(bad, monkeypatch):
    from reacherdistilation_amd import _native, student_mlp

    def no_native(*a, **k):
        raise AssertionError("native layer reached")
    monkeypatch.setattr(_native, "load", no_native)
    with pytest.raises(ValueError, match="dtype"):
        student_mlp.StudentMlpConfig(dtype=bad)
    cfg = student_mlp.StudentMlpConfig()
    cfg.dtype = bad   # set after construction: still caught, before the library is loaded
    with pytest.raises(ValueError, match="dtype"):
        student_mlp.StudentMlpTrainer(cfg, device="cuda:0")


def test_mlp_train_takes_the_dtype():
    import inspect

    from reacherdistilation_amd import mlp_train
    assert inspect.signature(mlp_train.train).parameters["dtype"].default == "f32"
    assert inspect.signature(mlp_train.train_envs).parameters["dtype"].default == "f32"
