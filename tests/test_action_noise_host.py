"""Host-side (no GPU) checks of the action noise in the students' closed loop
(include/reacher_action_noise.h): the NumPy model of tests/action_noise.py -- the expectation of the
GPU suites -- draws from a counter stream disjoint from the reset draws' and the coins', with the
moments of a standard normal over the seeds and shapes those suites use; every new name is exported
and declared; every rejection that needs no handle answers RD_EINVAL and names the function and the
field; the config structs keep their layouts; the Python layer checks its arguments."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import action_noise as an
from tests import envs_mix
from tests.conftest import ROOT

RD_EINVAL = -100000
FAKE = ctypes.c_void_p(0x1000)   # a non-NULL handle that a rejected call never dereferences


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, student_lstm, student_mlp  # noqa: F401  (register the symbols)
    build.build(verbose=False)
    return _native.load()


def _msg(lib):
    return lib.rd_last_error().decode()


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _nz(mode=an.FIXED, scale=1.0, seed=1):
    from reacherdistilation_amd._native import RdActionNoise
    return RdActionNoise(mode=mode, scale=scale, seed=seed)


# ---------------------------------------------------------------- the NumPy model
def test_counter_words_are_disjoint_from_the_coins_and_the_reset_draws():
    """word 3 = 0x40000000 | s: bit 30 set, bit 31 clear, for every step of an episode -- never the
    reset draws' 0 or 1, never a coin's 0x80000000 | s; and under one seed the words differ."""
    for s in range(an.EPISODE):
        w3 = int(an.counters(5, 3, 2, s)[3][0])
        assert w3 & 0x40000000 and not w3 & 0x80000000 and w3 not in (0, 1)
        assert w3 != (0x80000000 | s)
    from oracle import refnet_np as rn
    n, seed = 17, 11
    e = np.arange(n, dtype=np.uint64) + np.uint64(5)
    zeros = np.zeros(n, np.uint64)
    noise = rn.philox4x32_10(an.counters(5, n, 0, 0), seed, 0)
    reset = rn.philox4x32_10([e, e >> np.uint64(32), zeros, zeros], seed, 0)
    coin = rn.philox4x32_10([e, e >> np.uint64(32), zeros, np.full(n, 0x80000000, np.uint64)], seed, 0)
    assert not np.array_equal(noise[0], reset[0]) and not np.array_equal(noise[0], coin[0])
    # the coins of tests/envs_mix.py under the same seed are that other stream
    u = (coin[0] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(u < np.float32(0.5), envs_mix.teacher_coins(seed, 5, n, 0, 0, 0.5))


def test_draws_have_the_moments_of_a_standard_normal_over_the_gpu_runs_seeds():
    """83 envs x 100 steps x 2 draws = 16,600 samples: sample mean, variance and the cross-correlation of
    (xi0, xi1) within 4 / sqrt(N) of 0, 1, 0 (the mean's standard error is 1 / sqrt(N), the variance's
    sqrt(2 / N), the correlation's over N / 2 pairs sqrt(2 / N))."""
    seed, base, n, steps = an.RUNS[-1]
    xi = an.draw_table(seed, base, n, steps)
    assert xi.shape == (steps, n, 2) and xi.dtype == np.float32 and np.isfinite(xi).all()
    N = xi.size
    assert N == 16600
    bound = 4.0 / math.sqrt(N)
    x = xi.astype(np.float64)
    assert abs(x.mean()) < bound
    assert abs(x.var() - 1.0) < bound
    assert abs(np.corrcoef(x[..., 0].ravel(), x[..., 1].ravel())[0, 1]) < bound


def test_draws_are_a_function_of_seed_env_episode_and_step_alone():
    a = an.draw_table(11, 5, 17, 100)
    assert np.array_equal(a[:, 3:7], an.draw_table(11, 8, 4, 100))
    assert np.array_equal(a[50:], an.draw_table(11, 5, 17, 50, start=50))
    assert not np.array_equal(a, an.draw_table(12, 5, 17, 100))
    assert not np.array_equal(a[:50], a[50:])   # the episode enters
    wide = an.normal_draws(an.WIDE_SEED, an.WIDE_BASE, 83, 3, 49)
    assert np.isfinite(wide).all()
    assert not np.array_equal(wide, an.normal_draws(an.WIDE_SEED & 0xFFFFFFFF, an.WIDE_BASE, 83, 3, 49))   # the key's high word
    assert not np.array_equal(wide[40:], an.normal_draws(an.WIDE_SEED, an.WIDE_BASE + 40 - 2 ** 32, 43, 3, 49))   # the id's


def test_perturb_model_end_points():
    rs = np.random.RandomState(0)
    p = rs.uniform(-1, 1, (9, 4)).astype(np.float32)
    xi = an.normal_draws(3, 0, 9, 0, 0)
    assert np.array_equal(an.perturb(p, xi, an.NONE, 2.0), p[:, :2])
    assert np.array_equal(an.perturb(p, xi, an.FIXED, 0.0), p[:, :2])
    assert np.allclose(an.perturb(p, xi, an.FIXED, 0.5), p[:, :2] + 0.5 * xi, atol=1e-6)
    assert np.allclose(an.perturb(p, xi, an.POLICY, 1.0), p[:, :2] + np.exp(p[:, 2:]) * xi, atol=1e-5)


# ---------------------------------------------------------------- the ABI
NZ = r"const rd_action_noise\* nz"
@pytest.mark.parametrize("header,decl", [   # noqa: E302
    ("reacher_action_noise.h", r"int rd_perturb_actions\(" + NZ + r", int64_t env_base, int64_t n, int32_t episode, "
                               r"int32_t step,\s+const float\* pdflat , float\* actions , float\* xi ,\s+int device, "
                               r"void\* hip_stream\);"),
    ("reacher_student_mlp.h", r"int rdm_envs_set_action_noise\(rdm_trainer\* t, " + NZ + r"\);"),
    ("reacher_student_mlp.h", r"int rdm_envs_action_noise\(const rdm_trainer\* t, rd_action_noise\* out\);"),
    ("reacher_student_mlp.h", r"int rdm_envs_bind_actions\(rdm_trainer\* t, float\* buf , int64_t rows\);"),
    ("reacher_student_mlp.h", r"int rdm_evaluate_noisy\(rdm_trainer\* t, const rdm_eval_config\* cfg, " + NZ +
                              r",\s+float\* returns, float\* final_dist, float\* records\);"),
    ("reacher_student_lstm.h", r"int rdl_envs_set_action_noise\(rdl_trainer\* t, " + NZ + r"\);"),
    ("reacher_student_lstm.h", r"int rdl_envs_action_noise\(const rdl_trainer\* t, rd_action_noise\* out\);"),
    ("reacher_student_lstm.h", r"int rdl_envs_bind_actions\(rdl_trainer\* t, float\* buf , int64_t rows\);"),
    ("reacher_student_lstm.h", r"int rdl_evaluate_noisy\(rdl_trainer\* t, const rdl_eval_config\* cfg, " + NZ +
                               r", const float\* state0,\s+float\* returns, float\* final_dist, float\* records, "
                               r"float\* state_out\);"),
])
def test_exported_and_declared(lib, header, decl):
    name = re.search(r"(rd\w+)\\\(", decl).group(1)
    assert getattr(lib, name) is not None
    from reacherdistilation_amd import _native
    assert name in _native.SIGNATURES
    assert re.search(decl, _header(header)), name


def test_header_defines_the_modes_the_struct_and_the_stream():
    txt = open(os.path.join(ROOT, "include", "reacher_action_noise.h")).read()
    for word in ("#define RD_NOISE_NONE   0", "#define RD_NOISE_POLICY 1", "#define RD_NOISE_FIXED  2",
                 "typedef struct", "int32_t mode;", "float scale;", "uint64_t seed;", "} rd_action_noise;",
                 "0x40000000 | s", "Philox4x32-10", "fmaf(g_c, xi_c, mean_c)"):
        assert word in txt, word
    from reacherdistilation_amd._native import RdActionNoise
    from tests.test_product_hygiene import _c_layout
    c = _c_layout("rd_action_noise", "reacher_action_noise.h", [f[0] for f in RdActionNoise._fields_])
    assert c["sizeof"] == ctypes.sizeof(RdActionNoise) == 16
    for name in ("reacher_student_mlp.h", "reacher_student_lstm.h"):
        txt = " ".join(open(os.path.join(ROOT, "include", name)).read().replace("\n *", " ").split())
        for word in ("captured call keeps the values", "the same launch of the same kernel", "never reads"):
            assert word in txt, (name, word)


BAD_NOISE = [(dict(mode=3), "mode"), (dict(mode=-1), "mode"), (dict(scale=math.nan), "scale"),
             (dict(scale=-0.5), "scale"), (dict(scale=math.inf), "scale")]


def test_perturb_actions_rejects_before_any_device_call(lib):
    raw = (ctypes.c_float * 64)()
    p = ctypes.cast(raw, ctypes.c_void_p)
    fn = lib.rd_perturb_actions
    good = dict(nz=ctypes.byref(_nz()), env_base=0, n=4, episode=0, step=0, pdflat=p, actions=p, xi=None)
    cases = [(dict(nz=None), "null rd_action_noise"), (dict(pdflat=None), "null pdflat"), (dict(actions=None), "null actions"),
             (dict(n=0), "n "), (dict(env_base=-1), "env_base"), (dict(episode=-1), "episode"), (dict(step=-1), "step"),
             (dict(step=50), "step")]
    cases += [(dict(nz=ctypes.byref(_nz(**kw))), word) for kw, word in BAD_NOISE]
    for change, word in cases:
        a = dict(good, **change)
        rc = fn(a["nz"], a["env_base"], a["n"], a["episode"], a["step"], a["pdflat"], a["actions"], a["xi"], 0, None)
        assert rc == RD_EINVAL, change
        assert "rd_perturb_actions:" in _msg(lib) and word in _msg(lib), (change, _msg(lib))
    del raw


@pytest.mark.parametrize("prefix", ["rdm", "rdl"])
def test_setters_reject_before_the_handle_is_read(lib, prefix):
    fn = f"{prefix}_envs_set_action_noise"
    call = getattr(lib, fn)
    assert call(None, ctypes.byref(_nz())) == RD_EINVAL
    assert fn + ":" in _msg(lib) and "null trainer" in _msg(lib)
    assert call(FAKE, None) == RD_EINVAL
    assert fn + ":" in _msg(lib) and "null rd_action_noise" in _msg(lib)
    for kw, word in BAD_NOISE:
        assert call(FAKE, ctypes.byref(_nz(**kw))) == RD_EINVAL, kw
        assert fn + ":" in _msg(lib) and word in _msg(lib), (kw, _msg(lib))
    out = _nz()
    get = f"{prefix}_envs_action_noise"
    assert getattr(lib, get)(None, ctypes.byref(out)) == RD_EINVAL and get + ":" in _msg(lib)
    assert getattr(lib, get)(FAKE, None) == RD_EINVAL and get + ":" in _msg(lib)
    bind = f"{prefix}_envs_bind_actions"
    assert getattr(lib, bind)(None, None, 0) == RD_EINVAL
    assert bind + ":" in _msg(lib) and "null trainer" in _msg(lib)


@pytest.mark.parametrize("prefix", ["rdm", "rdl"])
def test_evaluate_noisy_rejects_a_bad_noise_before_the_handle_is_read(lib, prefix):
    fn = f"{prefix}_evaluate_noisy"
    call = getattr(lib, fn)
    raw = (ctypes.c_float * 64)()
    p = ctypes.cast(raw, ctypes.c_void_p)
    tail = (p, None, None) if prefix == "rdm" else (None, p, None, None, None)
    cases = [(None, "null rd_action_noise"), (ctypes.byref(_nz(mode=an.NONE)), "RD_NOISE_NONE")]
    cases += [(ctypes.byref(_nz(**kw)), word) for kw, word in BAD_NOISE]
    for nz, word in cases:
        assert call(FAKE, None, nz, *tail) == RD_EINVAL, word   # a NULL config: never reached
        assert fn + ":" in _msg(lib) and word in _msg(lib), (word, _msg(lib))
    # a good noise reaches evaluate's own checks, under this function's name
    assert call(None, None, ctypes.byref(_nz()), *tail) == RD_EINVAL
    assert fn + ":" in _msg(lib) and "null trainer, config or returns" in _msg(lib)
    # and the plain function keeps its name in its messages
    plain = getattr(lib, f"{prefix}_evaluate")
    assert plain(None, None, *tail) == RD_EINVAL and f"{prefix}_evaluate:" in _msg(lib)
    del raw


def test_config_structs_are_unchanged():
    from reacherdistilation_amd.student_lstm import RdlConfig, RdlEnvsConfig, RdlEvalConfig
    from reacherdistilation_amd.student_mlp import RdmConfig, RdmEnvsConfig, RdmEvalConfig
    from tests.test_product_hygiene import _c_layout
    eval_fields = ["n_envs", "env_base", "seed", "episodes", "first_episode", "grid", "draws"]
    assert [f[0] for f in RdmEvalConfig._fields_] == eval_fields == [f[0] for f in RdlEvalConfig._fields_]
    for C, struct, header, size in [(RdmEvalConfig, "rdm_eval_config", "reacher_student_mlp.h", 48),
                                    (RdlEvalConfig, "rdl_eval_config", "reacher_student_lstm.h", 48),
                                    (RdmEnvsConfig, "rdm_envs_config", "reacher_student_mlp.h", 32),
                                    (RdlEnvsConfig, "rdl_envs_config", "reacher_student_lstm.h", 32),
                                    (RdmConfig, "rdm_config", "reacher_student_mlp.h", 48),
                                    (RdlConfig, "rdl_config", "reacher_student_lstm.h", None)]:
        c = _c_layout(struct, header, [f[0] for f in C._fields_])
        assert c["sizeof"] == ctypes.sizeof(C), struct
        if size is not None:
            assert c["sizeof"] == size, struct
        for name, _ in C._fields_:
            assert c[name] == getattr(C, name).offset, (struct, name)


# ---------------------------------------------------------------- Python
def test_python_layer_has_the_noise_and_checks_its_arguments():
    from reacherdistilation_amd import action_noise, evaluate, lstm_train, mlp_train
    from reacherdistilation_amd.student_lstm import StudentLstmTrainer
    from reacherdistilation_amd.student_mlp import StudentMlpTrainer
    assert action_noise.NOISE_MODES == an.MODES
    with pytest.raises(ValueError, match="mode"):
        action_noise.native("gaussian", 1.0, 0)
    for scale in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="scale"):
            action_noise.native("fixed", scale, 0)
    nz = action_noise.native("policy", 0.25, 2 ** 64 + 5)
    assert (nz.mode, nz.scale, nz.seed) == (an.POLICY, 0.25, 5)
    for cls in (StudentMlpTrainer, StudentLstmTrainer):
        sig = inspect.signature(cls.set_action_noise).parameters
        assert (sig["mode"].default, sig["scale"].default, sig["seed"].default) == ("none", 1.0, None)
        assert isinstance(cls.action_noise, property) and isinstance(cls.actions, property)
        assert inspect.signature(cls.attach_envs).parameters["actions"].default is False
        ev = inspect.signature(cls.evaluate).parameters
        assert (ev["noise"].default, ev["noise_scale"].default, ev["noise_seed"].default) == ("none", 1.0, None)
        # the checks come before any native call: no handle is needed to be refused
        with pytest.raises(ValueError, match="mode"):
            cls.set_action_noise(object(), "gaussian")
        with pytest.raises(ValueError, match="scale"):
            cls.set_action_noise(object(), "fixed", -0.1)
        with pytest.raises(ValueError, match="mode"):
            cls.evaluate(object(), 4, 1, noise="gaussian")
        with pytest.raises(ValueError, match="scale"):
            cls.evaluate(object(), 4, 1, noise="policy", noise_scale=-2.0)
    for fn in (evaluate.evaluate_student_mlp, evaluate.evaluate_student_lstm):
        p = inspect.signature(fn).parameters
        assert (p["noise"].default, p["noise_scale"].default, p["noise_seed"].default) == ("none", 1.0, None)
    for mod in (mlp_train, lstm_train):
        p = inspect.signature(mod.train_envs).parameters
        assert (p["noise"].default, p["noise_scale"].default) == ("none", 1.0)
        assert p["noise"].kind is inspect.Parameter.KEYWORD_ONLY
