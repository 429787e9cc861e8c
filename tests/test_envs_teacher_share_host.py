"""Host-side (no GPU) checks of DAgger's beta-mixture in the students' persistent envs: the ABI
(rdm_ / rdl_envs_set_teacher_share and their getters, rdm_envs_bind_stepped_with,
rd_replay_push_rows_flags) is exported and declared, every rejection that needs no handle answers
RD_EINVAL before the handle is read, the config structs keep their sizes, the drivers have the
schedule's keywords, and the NumPy coin helper of tests/envs_mix.py -- the expectation of the GPU
suites -- behaves at its end points and gives both actors inside one episode for every mixed run
those suites make."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import envs_mix
from tests.conftest import ROOT

RD_EINVAL = -100000
FAKE = ctypes.c_void_p(0x1000)   # a non-NULL handle that a rejected call never dereferences


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, replay, student_lstm, student_mlp  # noqa: F401  (register the symbols)
    build.build(verbose=False)
    return _native.load()


def _msg(lib):
    return lib.rd_last_error().decode()


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


@pytest.mark.parametrize("header,decl", [
    ("reacher_student_mlp.h", r"int rdm_envs_set_teacher_share\(rdm_trainer\* t, float beta, uint64_t coin_seed\);"),
    ("reacher_student_mlp.h", r"float rdm_envs_teacher_share\(const rdm_trainer\* t\);"),
    ("reacher_student_mlp.h", r"int rdm_envs_bind_stepped_with\(rdm_trainer\* t, float\* buf, int64_t rows\);"),
    ("reacher_student_lstm.h", r"int rdl_envs_set_teacher_share\(rdl_trainer\* t, float beta, uint64_t coin_seed\);"),
    ("reacher_student_lstm.h", r"float rdl_envs_teacher_share\(const rdl_trainer\* t\);"),
    ("reacher_student_mlp.h", r"int rd_replay_push_rows_flags\(rd_replay\* h, const float\* x, const float\* t_pdflat, "
                         r"const float\* s_pdflat,\s+const float\* reward, const float\* carry, int64_t steps, "
                         r"int64_t n_envs,\s+const float\* stepped_with_rows\);"),
])
def test_exported_and_declared(lib, header, decl):
    name = re.search(r"(rd\w+)\\\(", decl).group(1)
    assert getattr(lib, name) is not None
    assert re.search(decl, _header(header)), name


def test_headers_describe_the_coin_the_default_and_the_captured_call():
    for name in ("reacher_student_mlp.h", "reacher_student_lstm.h"):
        txt = open(os.path.join(ROOT, "include", name)).read()
        for word in ("0x80000000", "Philox4x32-10", "captured call keeps", "default beta = 0"):
            assert word in txt, (name, word)


@pytest.mark.parametrize("prefix", ["rdm", "rdl"])
def test_set_teacher_share_rejects_before_the_handle_is_read(lib, prefix):
    fn = f"{prefix}_envs_set_teacher_share"
    call = getattr(lib, fn)
    assert call(None, 0.5, 1) == RD_EINVAL
    assert fn in _msg(lib) and "null trainer" in _msg(lib)
    for beta in (math.nan, -0.25, 1.5, -math.inf, math.inf):
        assert call(FAKE, beta, 1) == RD_EINVAL, beta
        assert fn in _msg(lib) and "beta" in _msg(lib), (beta, _msg(lib))
    assert getattr(lib, f"{prefix}_envs_teacher_share")(None) == -1.0


def test_bind_and_push_flags_reject_null_arguments(lib):
    assert lib.rdm_envs_bind_stepped_with(None, None, 0) == RD_EINVAL
    assert "rdm_envs_bind_stepped_with" in _msg(lib) and "null trainer" in _msg(lib)
    raw = (ctypes.c_float * 64)()
    p = ctypes.cast(raw, ctypes.c_void_p)
    push = lib.rd_replay_push_rows_flags
    for args, word in [((None, p, p, p, p, p, 50, 1, p), "null handle"),
                       ((FAKE, None, p, p, p, p, 50, 1, p), "null x"),
                       ((FAKE, p, None, p, p, p, 50, 1, p), "null t_pdflat"),
                       ((FAKE, p, p, p, None, p, 50, 1, p), "null reward"),
                       ((FAKE, p, p, p, p, p, 50, 1, None), "null stepped_with_rows")]:
        assert push(*args) == RD_EINVAL, word
        assert "rd_replay_push_rows_flags:" in _msg(lib) and word in _msg(lib), (word, _msg(lib))
    # the scalar form keeps its name in its messages
    assert lib.rd_replay_push_rows(FAKE, None, p, p, p, p, 50, 1, 1.0) == RD_EINVAL
    assert "rd_replay_push_rows:" in _msg(lib) and "null x" in _msg(lib)
    del raw


def test_config_structs_keep_their_sizes():
    from reacherdistilation_amd.student_lstm import RdlConfig, RdlEnvsConfig
    from reacherdistilation_amd.student_mlp import ACT_WITH, EnvsResult, RdmConfig, RdmEnvsConfig
    from tests.test_product_hygiene import _c_layout
    for C, struct, header, size in [(RdmEnvsConfig, "rdm_envs_config", "reacher_student_mlp.h", 32),
                                    (RdlEnvsConfig, "rdl_envs_config", "reacher_student_lstm.h", 32),
                                    (RdmConfig, "rdm_config", "reacher_student_mlp.h", 48),
                                    (RdlConfig, "rdl_config", "reacher_student_lstm.h", None)]:
        c = _c_layout(struct, header, [f[0] for f in C._fields_])
        assert c["sizeof"] == ctypes.sizeof(C), struct
        if size is not None:
            assert c["sizeof"] == size, struct
    assert ACT_WITH == {"teacher": 0, "student": 1}
    assert list(EnvsResult.__dataclass_fields__) == ["x", "t_pdflat", "s_pdflat", "reward"]


def test_drivers_and_trainers_have_the_schedule():
    from reacherdistilation_amd import lstm_train, mlp_train
    from reacherdistilation_amd.driver_env import teacher_share
    from reacherdistilation_amd.student_lstm import StudentLstmTrainer
    from reacherdistilation_amd.student_mlp import StudentMlpTrainer
    for mod in (mlp_train, lstm_train):
        sig = inspect.signature(mod.train_envs)
        for k, v in (("beta0", 0.0), ("beta_decay", 1.0)):
            p = sig.parameters[k]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == v, (mod.__name__, k)
    for cls in (StudentMlpTrainer, StudentLstmTrainer):
        assert callable(cls.set_teacher_share) and isinstance(cls.teacher_share, property)
        assert inspect.signature(cls.set_teacher_share).parameters["seed"].default is None
    assert isinstance(StudentMlpTrainer.stepped_with, property)
    assert "flags" in inspect.signature(StudentMlpTrainer.attach_envs).parameters
    # beta0 beta_decay^(k - warmup), exactly 0 below 2^-24
    assert teacher_share(3, 3, 1.0, 0.9) == 1.0 and teacher_share(5, 3, 0.5, 0.5) == 0.125
    assert teacher_share(24, 0, 1.0, 0.5) == 2.0 ** -24 and teacher_share(25, 0, 1.0, 0.5) == 0.0
    assert teacher_share(7, 0, 0.0, 1.0) == 0.0


def test_coin_helper_end_points():
    for seed, base, n, steps in envs_mix.MLP_RUNS[:3]:
        assert not envs_mix.coin_table(seed, base, n, steps, 0.0).any()
        assert envs_mix.coin_table(seed, base, n, steps, 1.0).all()
    # a pure function of (seed, env, episode, step): env 5 + 3 of one table is env 8 + 0 of another
    a = envs_mix.coin_table(11, 5, 17, 100, 0.5)
    b = envs_mix.coin_table(11, 8, 4, 100, 0.5)
    assert np.array_equal(a[:, 3:7], b)
    assert np.array_equal(a[50:], envs_mix.coin_table(11, 5, 17, 50, 0.5, start=50))
    assert not np.array_equal(a, envs_mix.coin_table(12, 5, 17, 100, 0.5))
    # the stream is not the reset draws': counter word 3 differs (0x80000000 | s against 0, 1)
    from oracle import refnet_np as rn
    e = np.arange(17, dtype=np.uint64) + np.uint64(5)
    reset0 = rn.philox4x32_10([e, e >> np.uint64(32), np.zeros(17, np.uint64), np.zeros(17, np.uint64)], 11, 0)[0]
    coin0 = rn.philox4x32_10([e, e >> np.uint64(32), np.zeros(17, np.uint64), np.full(17, 0x80000000, np.uint64)], 11, 0)[0]
    assert not np.array_equal(reset0, coin0)


@pytest.mark.parametrize("run", envs_mix.MLP_RUNS + envs_mix.LSTM_RUNS)
def test_both_actors_occur_inside_one_episode_in_every_gpu_run(run):
    """The premise of the beta = 0.5 GPU comparisons: for some env, one episode holds a teacher step and
    a student step (else a mixed run could not tell the select from either end point)."""
    seed, base, n, steps = run
    coins = envs_mix.coin_table(seed, base, n, steps, envs_mix.BETA)
    ep = coins[:envs_mix.EPISODE]
    assert (ep.any(axis=0) & (~ep).any(axis=0)).any()
    assert 0.3 < coins.mean() < 0.7 or n * steps < 200
