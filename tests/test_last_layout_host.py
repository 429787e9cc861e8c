"""Host-side (no GPU) checks of rdd_last_layout (include/reacher_distill.h), the read-only report
of the layout the trainer's last rollout launch took: its argument checks answer before anything
is dereferenced, and distill.py binds it."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build, distill  # noqa: F401  (distill registers rdd_last_layout)
    build.build(verbose=False)
    return _native.load()


def test_null_arguments_are_rejected(lib):
    """No GPU and no trainer here: an answer at all shows that the check precedes every use."""
    RD_EINVAL = -100000
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    fake = ctypes.c_void_p(0x1000)   # a non-NULL trainer that a rejected call never dereferences
    assert lib.rdd_last_layout(None, out) == RD_EINVAL
    msg = lib.rd_last_error().decode()
    assert "rdd_last_layout" in msg and "null" in msg.lower()
    assert lib.rdd_last_layout(fake, None) == RD_EINVAL
    msg = lib.rd_last_error().decode()
    assert "rdd_last_layout" in msg and "null" in msg.lower()
    assert list(out) == [7, 7, 7, 7]   # a refused call writes nothing


def test_trainer_binds_the_call():
    from reacherdistilation_amd.distill import DistillTrainer
    assert callable(DistillTrainer.last_layout)
