"""Host-side (no GPU) checks of the reference student's persistent-env ABI (rdm_envs_attach,
rdm_envs_act, rdm_rollout_envs, rdm_step_envs; include/reacher_student_mlp.h): the ctypes mirror
matches the header field by field, rdm_config keeps its layout, and every argument check that needs
no handle answers before any device call and before the handle is read.  The checks that read the
handle (no envs attached, no teacher, steps x n_envs > 2^31) are in tests/test_student_mlp_envs_gpu.py.
The ISA scans of tests/test_product_hygiene.py cover student_mlp_envs_kernel with every other
function of the product."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

HEADER = "reacher_student_mlp.h"
RD_EINVAL = -100000
CALLS = ("rdm_envs_act", "rdm_rollout_envs", "rdm_step_envs")


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, student_mlp  # noqa: F401  (student_mlp registers the symbols)
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
    from reacherdistilation_amd.student_mlp import ACT_WITH, RdmEnvsConfig as C
    fields = [f[0] for f in C._fields_]
    assert fields == ["n_envs", "env_base", "seed", "grid"] == _header_fields("rdm_envs_config")
    c = _c_layout("rdm_envs_config", fields)
    assert c["sizeof"] == ctypes.sizeof(C) == 32
    for f in fields:
        assert c[f] == getattr(C, f).offset, f
        assert ctypes.sizeof(dict(C._fields_)[f]) == (4 if f == "grid" else 8), f
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    assert re.search(r"#define RDM_ACT_TEACHER 0\b", txt) and re.search(r"#define RDM_ACT_STUDENT 1\b", txt)
    assert ACT_WITH == {"teacher": 0, "student": 1}


def test_rdm_config_layout_is_unchanged():
    """The trainer's own config: the fields, offsets and size it had before the envs were added."""
    from reacherdistilation_amd.student_mlp import RdmConfig as C
    fields = ["loss", "lr", "beta1", "beta2", "eps", "grid", "metrics_len", "keep_prob", "seed", "row_base"]
    assert [f[0] for f in C._fields_] == fields == _header_fields("rdm_config")
    c = _c_layout("rdm_config", fields)
    assert c["sizeof"] == ctypes.sizeof(C) == 48
    want = dict(loss=0, lr=4, beta1=8, beta2=12, eps=16, grid=20, metrics_len=24, keep_prob=28, seed=32, row_base=40)
    for f in fields:
        assert c[f] == getattr(C, f).offset == want[f], f


def _msg(lib):
    return lib.rd_last_error().decode()


FAKE = ctypes.c_void_p(0x1000)   # a non-NULL trainer that a rejected call never dereferences


def test_attach_rejects_null_arguments_before_any_device_call(lib):
    """No GPU here: an answer at all shows that the check precedes every HIP call."""
    from reacherdistilation_amd.student_mlp import RdmEnvsConfig
    cfg = RdmEnvsConfig(n_envs=4)
    assert lib.rdm_envs_attach(None, ctypes.byref(cfg)) == RD_EINVAL
    assert "rdm_envs_attach" in _msg(lib) and "null trainer" in _msg(lib)
    assert lib.rdm_envs_attach(FAKE, None) == RD_EINVAL
    assert "rdm_envs_attach" in _msg(lib) and "null config" in _msg(lib)
    assert lib.rdm_envs_reset(None) == RD_EINVAL and "rdm_envs_reset" in _msg(lib)
    assert lib.rdm_envs_get_state(None, None, None, None) == RD_EINVAL and "rdm_envs_get_state" in _msg(lib)


@pytest.mark.parametrize("field,value", [("n_envs", 0), ("n_envs", -3), ("n_envs", 2 ** 31 + 1), ("env_base", -1),
                                         ("grid", -1)])
def test_attach_rejects_bad_config_values_before_any_device_call(lib, field, value):
    from reacherdistilation_amd.student_mlp import RdmEnvsConfig
    cfg = RdmEnvsConfig(n_envs=4)
    setattr(cfg, field, value)
    assert lib.rdm_envs_attach(FAKE, ctypes.byref(cfg)) == RD_EINVAL
    assert "rdm_envs_attach" in _msg(lib) and field in _msg(lib)


def _buffers():
    """16-byte aligned host floats standing in for x and t_pdflat (never dereferenced), and a view 4
    bytes into them."""
    raw = (ctypes.c_char * 160)()
    base = (ctypes.addressof(raw) + 15) & ~15
    return raw, ctypes.c_void_p(base), ctypes.c_void_p(base + 64), ctypes.c_void_p(base + 4)


@pytest.mark.parametrize("fn", CALLS)
def test_calls_reject_bad_arguments_before_any_device_call(lib, fn):
    """rdm_envs_act / rdm_rollout_envs / rdm_step_envs with a fake non-NULL handle: each message
    names the function and the field."""
    call = getattr(lib, fn)
    raw, x, t, off = _buffers()
    cases = [((None, 1, 1, x, t, None, None), "null trainer"),
             ((FAKE, 1, 1, None, t, None, None), "null x"),
             ((FAKE, 1, 1, x, None, None, None), "null t_pdflat"),
             ((FAKE, 1, 1, off, t, None, None), "x is not 16-byte aligned"),
             ((FAKE, 1, 1, x, off, None, None), "t_pdflat is not 16-byte aligned"),
             ((FAKE, 1, 0, x, t, None, None), "steps"),
             ((FAKE, 1, -4, x, t, None, None), "steps"),
             ((FAKE, 2, 1, x, t, None, None), "act_with"),
             ((FAKE, -1, 1, x, t, None, None), "act_with")]
    for args, word in cases:
        assert call(*args) == RD_EINVAL, word
        assert fn + ":" in _msg(lib) and word in _msg(lib), (word, _msg(lib))
    del raw


def test_train_envs_and_the_host_methods_exist():
    import inspect
    from reacherdistilation_amd import mlp_train
    from reacherdistilation_amd.student_mlp import EnvsResult, StudentMlpTrainer
    sig = inspect.signature(mlp_train.train_envs)
    assert list(sig.parameters)[:2] == ["n_envs", "opt_steps"]
    want = dict(keep_prob=1.0, loss="kl", lr=1e-4, accum_steps=50, warmup_steps=0, seed=0, teacher=None, eval_every=0)
    for k, v in want.items():
        p = sig.parameters[k]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == v, k
    assert {"device", "eval_envs"} <= set(sig.parameters)
    for name in ("attach_envs", "reset_envs", "act_envs", "rollout_envs", "step_envs", "env_state"):
        assert callable(getattr(StudentMlpTrainer, name)), name
    assert [f for f in EnvsResult.__dataclass_fields__] == ["x", "t_pdflat", "s_pdflat", "reward"]
