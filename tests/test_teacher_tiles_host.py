"""Host-side (no GPU) checks of rdd_config.teacher_tiles (include/reacher_distill.h): rdd_create
refuses a mask that is not built before it touches the device, and DistillConfig carries the field
with the library's default."""
import ctypes

import pytest

RD_EINVAL = -100000


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, distill  # noqa: F401  (distill registers rdd_create)
    build.build(verbose=False)
    return _native.load()


def _config(mask):
    from reacherdistilation_amd.distill import RddConfig
    return RddConfig(n_envs=64, n_envs_global=64, env_base=0, seed=0, loss=0, act_with=0, lr=1e-4, beta1=0.9,
                     beta2=0.999, eps=1e-8, grid=0, metrics_len=0, stagger=0, student_dtype=0, accum_steps=1,
                     f32_split=1, group_envs=0, teacher_tiles=mask)


@pytest.mark.parametrize("mask", [-2, 1, 0b0011, 0b0100, 0b0110, 0b1000, 0b1100, 0b1111, 0b10000])
def test_create_rejects_a_mask_that_is_not_built(lib, mask):
    """Tile 0 is never the consumer's, and only 0b0010, 0b1010 and 0b1110 are instantiated.  No GPU
    here: an answer at all shows that the check precedes every device call."""
    h = ctypes.c_void_p()
    c = _config(mask)
    assert lib.rdd_create(ctypes.byref(h), ctypes.byref(c), 0, None) == RD_EINVAL
    msg = lib.rd_last_error().decode()
    assert "rdd_create" in msg and "teacher_tiles" in msg and str(mask) in msg, msg
    assert not h.value


def test_config_default_is_the_library_default():
    from reacherdistilation_amd.distill import DistillConfig, RddConfig
    assert DistillConfig().teacher_tiles == -1
    assert RddConfig._fields_[-1][0] == "teacher_tiles"   # appended: older callers' zeroed tail means 0, the parent's layout
