"""Host-side (no GPU) checks of the reference student's whole-episode evaluation ABI (rdm_evaluate,
include/reacher_student_mlp.h): the ctypes mirror matches the header field by field, and the
argument checks answer before any device call and before the handle is read.  The ISA scans of
tests/test_product_hygiene.py cover student_mlp_evaluate_kernel with every other function of the
product."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

HEADER, STRUCT = "reacher_student_mlp.h", "rdm_eval_config"
RD_EINVAL = -100000


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, student_mlp  # noqa: F401  (student_mlp registers rdm_evaluate)
    build.build(verbose=False)
    return _native.load()


def _c_layout(fields):
    """sizeof and offsetof of the header's struct, compiled with gcc from the header itself."""
    body = "\n".join(f'printf("{f} %zu\\n", offsetof({STRUCT}, {f}));' for f in fields)
    src = (f'#include <stddef.h>\n#include <stdio.h>\n#include "{HEADER}"\n'
           f'int main(void) {{ printf("sizeof %zu\\n", sizeof({STRUCT})); {body} return 0; }}\n')
    d = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(d, exist_ok=True)
    c, exe = os.path.join(d, f"layout_{STRUCT}.c"), os.path.join(d, f"layout_{STRUCT}")
    with open(c, "w") as fh:
        fh.write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in res.splitlines())}


def test_eval_config_mirror_matches_the_header():
    from reacherdistilation_amd.student_mlp import RdmEvalConfig as C
    fields = [f[0] for f in C._fields_]
    c = _c_layout(fields)
    assert c["sizeof"] == ctypes.sizeof(C)
    for f in fields:
        assert c[f] == getattr(C, f).offset, f
        assert ctypes.sizeof(dict(C._fields_)[f]) == {"n_envs": 8, "env_base": 8, "seed": 8, "draws": 8}.get(f, 4), f
    # every member of the C struct is mirrored, in the header's order
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + STRUCT + ";", txt).group(1)
    assert re.findall(r"(\w+)\s*(?:,|;)", body) == fields
    # rdd_eval_config without `policy`
    from reacherdistilation_amd.distill import RddEvalConfig
    assert fields == [f[0] for f in RddEvalConfig._fields_ if f[0] != "policy"]


def _msg(lib):
    return lib.rd_last_error().decode()


def test_null_arguments_are_rejected_before_any_device_call(lib):
    """No GPU here: an answer at all shows that the check precedes every HIP call."""
    from reacherdistilation_amd.student_mlp import RdmEvalConfig
    cfg = RdmEvalConfig(n_envs=4, episodes=1)
    out = (ctypes.c_float * 4)()
    fake = ctypes.c_void_p(0x1000)   # a non-NULL trainer that a rejected call never dereferences
    assert lib.rdm_evaluate(None, ctypes.byref(cfg), out, None, None) == RD_EINVAL
    assert "rdm_evaluate" in _msg(lib) and "null" in _msg(lib).lower()
    assert lib.rdm_evaluate(fake, None, out, None, None) == RD_EINVAL
    assert "rdm_evaluate" in _msg(lib) and "null" in _msg(lib).lower()
    assert lib.rdm_evaluate(fake, ctypes.byref(cfg), None, None, None) == RD_EINVAL
    assert "rdm_evaluate" in _msg(lib) and "null" in _msg(lib).lower()
    v = (ctypes.c_float * 16)()
    for args in ((None, v, v, v), (fake, None, v, v), (fake, v, None, v), (fake, v, v, None)):
        assert lib.rdm_set_teacher(*args) == RD_EINVAL
        assert "rdm_set_teacher" in _msg(lib) and "null" in _msg(lib).lower()


@pytest.mark.parametrize("field,value,word", [("n_envs", 0, "n_envs"), ("n_envs", -3, "n_envs"),
                                              ("episodes", 0, "episodes"), ("episodes", -1, "episodes"),
                                              ("env_base", -1, "env_base"), ("first_episode", -1, "first_episode"),
                                              ("grid", -1, "grid")])
def test_bad_config_values_are_rejected_before_any_device_call(lib, field, value, word):
    from reacherdistilation_amd.student_mlp import RdmEvalConfig
    cfg = RdmEvalConfig(n_envs=4, episodes=1)
    setattr(cfg, field, value)
    out = (ctypes.c_float * 4)()
    assert lib.rdm_evaluate(ctypes.c_void_p(0x1000), ctypes.byref(cfg), out, None, None) == RD_EINVAL
    assert "rdm_evaluate" in _msg(lib) and word in _msg(lib)


def test_evaluate_module_lists_the_student_mlp_evaluation():
    from reacherdistilation_amd import evaluate
    assert "evaluate_student_mlp" in evaluate.__all__ and callable(evaluate.evaluate_student_mlp)
    assert {"evaluate_policy", "collect_episodes", "gym_draw_table"} <= set(evaluate.__all__)
