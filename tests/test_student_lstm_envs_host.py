"""Host-side (no GPU) checks of the LSTM student's persistent-env ABI (rdl_envs_attach, rdl_envs_act,
rdl_rollout_envs, rdl_step_envs, rdl_envs_get_state, rdl_envs_get_query_state;
include/reacher_student_lstm.h): the ctypes mirror matches the header field by field, rdl_config keeps
its layout, and every argument check that needs no handle answers before any device call and before
the handle is read.  The checks that read the handle (no envs attached, no teacher, T > 16, steps % 50,
B > max_windows) are in tests/test_student_lstm_envs_gpu.py.  The ISA scans of
tests/test_product_hygiene.py cover student_lstm_envs_kernel with every other function of the product."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

HEADER = "reacher_student_lstm.h"
RD_EINVAL = -100000
TRAIN_CALLS = ("rdl_rollout_envs", "rdl_step_envs")
SYMBOLS = ("rdl_envs_attach", "rdl_envs_reset", "rdl_envs_act", "rdl_rollout_envs", "rdl_step_envs",
           "rdl_envs_get_state", "rdl_envs_get_query_state")


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, student_lstm  # noqa: F401  (student_lstm registers the symbols)
    build.build(verbose=False)
    return _native.load()


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


def _header_fields(struct):
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct + ";", txt).group(1)
    return re.findall(r"(\w+)\s*(?:,|;)", body)


def test_envs_config_mirror_matches_the_header():
    from reacherdistilation_amd.student_lstm import ACT_WITH, RdlEnvsConfig as C
    fields = [f[0] for f in C._fields_]
    assert fields == ["n_envs", "env_base", "seed", "grid"] == _header_fields("rdl_envs_config")
    c = _c_layout("rdl_envs_config", fields)
    assert c["sizeof"] == ctypes.sizeof(C) == 32
    for f in fields:
        assert c[f] == getattr(C, f).offset, f
        assert ctypes.sizeof(dict(C._fields_)[f]) == (4 if f == "grid" else 8), f


def test_act_with_values():
    from reacherdistilation_amd.student_lstm import ACT_WITH
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    assert re.search(r"#define RDL_ACT_TEACHER 0\b", txt) and re.search(r"#define RDL_ACT_STUDENT 1\b", txt)
    assert ACT_WITH == {"teacher": 0, "student": 1}


def test_rdl_config_layout_is_unchanged():
    """The trainer's own config: the fields, offsets and size it had before the envs were added."""
    from reacherdistilation_amd.student_lstm import RdlConfig as C
    fields = ["loss", "lr", "beta1", "beta2", "eps", "steps", "max_windows", "metrics_len", "keep_prob", "seed",
              "row_base", "kernels"]
    assert [f[0] for f in C._fields_] == fields == _header_fields("rdl_config")
    c = _c_layout("rdl_config", fields)
    assert c["sizeof"] == ctypes.sizeof(C) == 64
    want = dict(loss=0, lr=4, beta1=8, beta2=12, eps=16, steps=20, max_windows=24, metrics_len=28, keep_prob=32,
                seed=40, row_base=48, kernels=56)
    for f in fields:
        assert c[f] == getattr(C, f).offset == want[f], f


def test_new_symbols_are_exported(lib):
    from reacherdistilation_amd import _native
    have = _native.exported_symbols()
    for name in SYMBOLS:
        assert have.get(name) is True, name
        assert getattr(lib, name).argtypes is not None, name


def _msg(lib):
    return lib.rd_last_error().decode()


FAKE = ctypes.c_void_p(0x1000)   # a non-NULL trainer that a rejected call never dereferences


def test_attach_rejects_null_arguments_before_any_device_call(lib):
    """No GPU here: an answer at all shows that the check precedes every HIP call."""
    from reacherdistilation_amd.student_lstm import RdlEnvsConfig
    cfg = RdlEnvsConfig(n_envs=4)
    assert lib.rdl_envs_attach(None, ctypes.byref(cfg)) == RD_EINVAL
    assert "rdl_envs_attach" in _msg(lib) and "null trainer" in _msg(lib)
    assert lib.rdl_envs_attach(FAKE, None) == RD_EINVAL
    assert "rdl_envs_attach" in _msg(lib) and "null config" in _msg(lib)
    assert lib.rdl_envs_reset(None) == RD_EINVAL and "rdl_envs_reset" in _msg(lib)
    assert lib.rdl_envs_get_state(None, None, None, None) == RD_EINVAL and "rdl_envs_get_state" in _msg(lib)
    assert lib.rdl_envs_get_state(FAKE, None, None, None) == RD_EINVAL and "rdl_envs_get_state" in _msg(lib)
    assert lib.rdl_envs_get_query_state(None, None) == RD_EINVAL and "rdl_envs_get_query_state" in _msg(lib)
    assert lib.rdl_envs_get_query_state(FAKE, None) == RD_EINVAL and "rdl_envs_get_query_state" in _msg(lib)


@pytest.mark.parametrize("field,value", [("n_envs", 0), ("n_envs", -3), ("n_envs", 2 ** 31 + 1), ("env_base", -1),
                                         ("grid", -1)])
def test_attach_rejects_bad_config_values_before_any_device_call(lib, field, value):
    from reacherdistilation_amd.student_lstm import RdlEnvsConfig
    cfg = RdlEnvsConfig(n_envs=4)
    setattr(cfg, field, value)
    assert lib.rdl_envs_attach(FAKE, ctypes.byref(cfg)) == RD_EINVAL
    assert "rdl_envs_attach" in _msg(lib) and field in _msg(lib)


def _buffers():
    """Host floats standing in for records and the three window buffers (never dereferenced)."""
    raw = (ctypes.c_char * 256)()
    base = ctypes.addressof(raw)
    return raw, [ctypes.c_void_p(base + 64 * k) for k in range(4)]


def test_act_rejects_bad_arguments_before_any_device_call(lib):
    """rdl_envs_act with a fake non-NULL handle: each message names the function and the field."""
    raw, (rec, ob, pv, tw) = _buffers()
    cases = [((None, 1, 1, rec, None, None, None, None, 0), "null trainer"),
             ((FAKE, 1, 1, None, None, None, None, None, 0), "null records"),
             ((FAKE, 1, 0, rec, None, None, None, None, 0), "steps"),
             ((FAKE, 1, -4, rec, None, None, None, None, 0), "steps"),
             ((FAKE, 2, 1, rec, None, None, None, None, 0), "act_with"),
             ((FAKE, -1, 1, rec, None, None, None, None, 0), "act_with"),
             ((FAKE, 1, 50, rec, None, ob, None, tw, 41), "prev_w"),
             ((FAKE, 1, 50, rec, None, None, pv, tw, 41), "ob_w"),
             ((FAKE, 1, 50, rec, None, ob, pv, None, 41), "t_w"),
             ((FAKE, 1, 50, rec, None, ob, pv, tw, 0), "windows")]
    for args, word in cases:
        assert lib.rdl_envs_act(*args) == RD_EINVAL, word
        assert "rdl_envs_act:" in _msg(lib) and word in _msg(lib), (word, _msg(lib))
    del raw


@pytest.mark.parametrize("fn", TRAIN_CALLS)
def test_training_calls_reject_bad_arguments_before_any_device_call(lib, fn):
    call = getattr(lib, fn)
    raw, (rec, ob, pv, tw) = _buffers()
    cases = [((None, 1, 50, rec, None, ob, pv, tw), "null trainer"),
             ((FAKE, 1, 50, None, None, ob, pv, tw), "null records"),
             ((FAKE, 1, 0, rec, None, ob, pv, tw), "steps"),
             ((FAKE, 1, -50, rec, None, ob, pv, tw), "steps"),
             ((FAKE, 2, 50, rec, None, ob, pv, tw), "act_with"),
             ((FAKE, -1, 50, rec, None, ob, pv, tw), "act_with"),
             ((FAKE, 1, 50, rec, None, None, None, None), "ob_w"),
             ((FAKE, 1, 50, rec, None, ob, None, tw), "prev_w"),
             ((FAKE, 1, 50, rec, None, ob, pv, None), "t_w")]
    for args, word in cases:
        assert call(*args) == RD_EINVAL, word
        assert fn + ":" in _msg(lib) and word in _msg(lib), (word, _msg(lib))
    del raw


def test_train_envs_and_the_host_methods_exist():
    import inspect
    from reacherdistilation_amd import lstm_train
    from reacherdistilation_amd.student_lstm import EnvsResult, StudentLstmTrainer
    sig = inspect.signature(lstm_train.train_envs)
    assert list(sig.parameters)[:2] == ["n_envs", "opt_steps"]
    want = dict(keep_prob=1.0, loss="kl", lr=1e-3, accum_steps=50, warmup_steps=0, seed=0, teacher=None, eval_every=0)
    for k, v in want.items():
        p = sig.parameters[k]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == v, k
    assert {"device", "eval_envs"} <= set(sig.parameters)
    for name in ("attach_envs", "reset_envs", "act_envs", "rollout_envs", "step_envs", "env_state", "query_state"):
        assert callable(getattr(StudentLstmTrainer, name)), name
    assert inspect.signature(StudentLstmTrainer.attach_envs).parameters["accum_steps"].default == 50
    assert [f for f in EnvsResult.__dataclass_fields__] == ["records", "reward", "ob_w", "prev_w", "t_w"]
