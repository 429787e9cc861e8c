"""Host-side (no GPU) checks of the LSTM student's whole-episode evaluation ABI (rdl_evaluate,
include/reacher_student_lstm.h): the ctypes mirror matches the header field by field and equals
rdm_eval_config's, and the argument checks answer before any device call and before the handle is
read.  The ISA scans of tests/test_product_hygiene.py cover student_lstm_evaluate_kernel and
lstm_eval_pack_kernel with every other function of the product."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

HEADER, STRUCT = "reacher_student_lstm.h", "rdl_eval_config"
RD_EINVAL = -100000


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, student_lstm  # noqa: F401  (student_lstm registers rdl_evaluate)
    build.build(verbose=False)
    return _native.load()


def _c_layout(fields):
    """sizeof and offsetof of the header's struct, compiled with gcc from the header itself."""
    body = "\n".join(f'printf("{f} %zu\\n", offsetof({STRUCT}, {f}));' for f in fields)
    src = (f'#include <stddef.h>\n#include <stdio.h>\n#include "{HEADER}"\n'
           f'int main(void) {{ printf("sizeof %zu\\n", sizeof({STRUCT})); {body} '
           f'printf("max_steps %d\\n", RDL_EVAL_MAX_STEPS); return 0; }}\n')
    d = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(d, exist_ok=True)
    c, exe = os.path.join(d, f"layout_{STRUCT}.c"), os.path.join(d, f"layout_{STRUCT}")
    with open(c, "w") as fh:
        fh.write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in res.splitlines())}


def test_eval_config_mirror_matches_the_header():
    from reacherdistilation_amd.student_lstm import RdlEvalConfig as C
    fields = [f[0] for f in C._fields_]
    c = _c_layout(fields)
    assert c["sizeof"] == ctypes.sizeof(C)
    for f in fields:
        assert c[f] == getattr(C, f).offset, f
        assert ctypes.sizeof(dict(C._fields_)[f]) == {"n_envs": 8, "env_base": 8, "seed": 8, "draws": 8}.get(f, 4), f
    assert c["max_steps"] >= 16   # the documented history bound covers the issue's T = 16
    # every member of the C struct is mirrored, in the header's order
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + STRUCT + ";", txt).group(1)
    assert re.findall(r"(\w+)\s*(?:,|;)", body) == fields


def test_eval_config_equals_the_mlp_students():
    from reacherdistilation_amd.student_lstm import RdlEvalConfig
    from reacherdistilation_amd.student_mlp import RdmEvalConfig
    assert [(n, t) for n, t in RdlEvalConfig._fields_] == [(n, t) for n, t in RdmEvalConfig._fields_]
    assert ctypes.sizeof(RdlEvalConfig) == ctypes.sizeof(RdmEvalConfig)
    for n, _ in RdlEvalConfig._fields_:
        assert getattr(RdlEvalConfig, n).offset == getattr(RdmEvalConfig, n).offset, n


def _msg(lib):
    return lib.rd_last_error().decode()


def test_null_arguments_are_rejected_before_any_device_call(lib):
    """No GPU here: an answer at all shows that the check precedes every HIP call."""
    from reacherdistilation_amd.student_lstm import RdlEvalConfig
    cfg = RdlEvalConfig(n_envs=4, episodes=1)
    out = (ctypes.c_float * 4)()
    fake = ctypes.c_void_p(0x1000)   # a non-NULL trainer that a rejected call never dereferences
    assert lib.rdl_evaluate(None, ctypes.byref(cfg), None, out, None, None, None) == RD_EINVAL
    assert "rdl_evaluate" in _msg(lib) and "null" in _msg(lib).lower()
    assert lib.rdl_evaluate(fake, None, None, out, None, None, None) == RD_EINVAL
    assert "rdl_evaluate" in _msg(lib) and "null" in _msg(lib).lower()
    assert lib.rdl_evaluate(fake, ctypes.byref(cfg), None, None, None, None, None) == RD_EINVAL
    assert "rdl_evaluate" in _msg(lib) and "null" in _msg(lib).lower()


def test_set_teacher_rejects_nulls(lib):
    fake = ctypes.c_void_p(0x1000)
    v = (ctypes.c_float * 16)()
    for args in ((None, v, v, v), (fake, None, v, v), (fake, v, None, v), (fake, v, v, None)):
        assert lib.rdl_set_teacher(*args) == RD_EINVAL
        assert "rdl_set_teacher" in _msg(lib) and "null" in _msg(lib).lower()


@pytest.mark.parametrize("field,value,word", [("n_envs", 0, "n_envs"), ("n_envs", -3, "n_envs"),
                                              ("n_envs", 2 ** 31 + 1, "n_envs"),
                                              ("episodes", 0, "episodes"), ("episodes", -1, "episodes"),
                                              ("env_base", -1, "env_base"), ("first_episode", -1, "first_episode"),
                                              ("grid", -1, "grid")])
def test_bad_config_values_are_rejected_before_any_device_call(lib, field, value, word):
    from reacherdistilation_amd.student_lstm import RdlEvalConfig
    cfg = RdlEvalConfig(n_envs=4, episodes=1)
    setattr(cfg, field, value)
    out = (ctypes.c_float * 4)()
    assert lib.rdl_evaluate(ctypes.c_void_p(0x1000), ctypes.byref(cfg), None, out, None, None, None) == RD_EINVAL
    assert "rdl_evaluate" in _msg(lib) and word in _msg(lib)


def test_evaluate_module_lists_the_student_lstm_evaluation():
    from reacherdistilation_amd import evaluate
    assert "evaluate_student_lstm" in evaluate.__all__ and callable(evaluate.evaluate_student_lstm)
    assert {"evaluate_policy", "evaluate_student_mlp", "collect_episodes", "gym_draw_table"} <= set(evaluate.__all__)
