"""Host-side (no GPU) checks of the PPO trainer's kickstarting (include/reacher_ppo.h: a teacher's
KL term in the minibatch loss): the new exports and their ctypes signatures, rdp_config's unchanged
layout, and the tests' own restatement of the KL gradient (tests/ppo_kickstart.py), which the GPU
tests hold the kernel to, against central finite differences and against policy_np's pinned kl_loss.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import policy_np as pn
from oracle import ppo_np as pp
from tests import ppo_kickstart as ks
from tests import ppo_parity as par
from tests.conftest import ROOT

P, I64, F32, INT, F64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int, ctypes.c_double
EXPORTS = {
    "rdp_set_teacher": (INT, [P, P, P, P]),
    "rdp_set_distill": (INT, [P, F32, I64]),
    "rdp_distill_coef": (F32, [P]),
    "rdp_get_teacher_labels": (INT, [P, P]),
    "rdp_read_distill_metrics": (INT, [P, I64, P]),
    "rdp_set_obfilter": (INT, [P, P, P, F64]),
}
C_TYPES = {"int": INT, "float": F32, "double": F64, "int64_t": I64}


@pytest.fixture(scope="module")
def lib():
    from reacherdistilation_amd import _native, build
    import reacherdistilation_amd.ppo  # noqa: F401  (registers the rdp_* signatures)
    build.build(verbose=False)
    return _native.load()


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_export_is_present_with_the_headers_signature(lib, name):
    """The symbol is in the library, the binding's restype / argtypes are the ones stated here, and
    both agree with the declaration in include/reacher_ppo.h (pointers -> void*)."""
    fn = getattr(lib, name)
    res, args = EXPORTS[name]
    assert fn.restype is res and list(fn.argtypes) == args
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "reacher_ppo.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\((.*?)\);", txt, re.S)
    assert m, name

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return P
        return C_TYPES[decl.replace("const ", "").split()[0]]

    assert ctype(m.group(1)) is res
    assert [ctype(d) for d in m.group(2).split(",")] == args


def test_config_layout_is_unchanged():
    from reacherdistilation_amd.ppo import RdpConfig
    assert ctypes.sizeof(RdpConfig) == 80
    assert [f[0] for f in RdpConfig._fields_] == [
        "n_envs", "horizon", "seed", "env_base", "clip_param", "entcoeff", "optim_epochs", "optim_stepsize",
        "optim_batchsize", "gamma", "lam", "schedule_linear", "max_timesteps", "metrics_len"]
    assert RdpConfig.metrics_len.offset == 72


def _case(n=7, seed=0):
    b = par.synthetic_batch(n, 1, seed)
    pol = b["pol"].astype(np.float64)
    pol[-2:] = (0.15, -0.2)                                          # a log-std of the learner's own
    rs = np.random.RandomState(seed + 7)
    pol[slice(*par.block("W3"))] += rs.uniform(-.3, .3, 128)         # means that differ from the teacher's
    tpol, tmean, tstd = ks.teacher()
    ob = rs.standard_normal((n, pp.OBD))                             # raw observations; the learner's filter is
    lmean, lstd = rs.uniform(-.2, .2, pp.OBD), rs.uniform(.6, 1.5, pp.OBD)   # not the teacher's
    return pol, pp.obz(ob, lmean, lstd), ob, (tpol, tmean, tstd), ks.teacher_pdflat(tpol, tmean, tstd, ob)


def test_kl_gradient_restatement_matches_finite_differences():
    """lam x mean KL at n = 7 rows, f64: central differences over every policy entry (h = 1e-6)
    agree with kl_grad to 1e-7 of the largest entry; the teacher's clipped input is exercised."""
    lam = 0.7
    pol, z, ob, (tpol, tmean, tstd), tflat = _case()
    assert (np.abs((ob - tmean) / tstd) > 5).any()
    g = ks.kl_grad(pol, z, tflat, lam)
    assert g.shape == (pp.P_POL,) and np.abs(g[-2:]).min() > 1e-3 and np.abs(g[:704]).max() > 1e-4
    fd = np.zeros_like(g)
    h = 1e-6
    for e in range(pp.P_POL):
        p1, p0 = pol.copy(), pol.copy()
        p1[e] += h
        p0[e] -= h
        fd[e] = lam * (ks.kl_heads(p1, z, tflat, 1.0)[0] - ks.kl_heads(p0, z, tflat, 1.0)[0]) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-7 * np.abs(g).max(), np.abs(fd - g).max() / np.abs(g).max()


def test_kl_restatement_matches_policy_np_up_to_the_minibatch_mean():
    """policy_np.loss_and_dmean(..., "kl") is the pinned kl_loss: its loss is the sum over the rows,
    its dmean and dlogstd carry no 1/mb.  kl_heads is that times lam / mb."""
    lam = 0.7
    pol, z, ob, (tpol, tmean, tstd), tflat = _case()
    n = z.shape[0]
    fs = pp.pol_forward(pol, z)
    ft = pn.forward(tpol.astype(np.float64), tmean.astype(np.float64), tstd.astype(np.float64), ob)
    np.testing.assert_array_equal(np.concatenate([ft["mean"], np.tile(ft["logstd"], (n, 1))], 1), tflat)
    kl_sum, dmean, dls, _ = pn.loss_and_dmean(fs, ft, "kl", n)
    kl_mean, dmean_k, dls_rows, _ = ks.kl_heads(pol, z, tflat, lam)
    assert kl_mean == pytest.approx(kl_sum / n, rel=1e-14)
    np.testing.assert_allclose(dmean_k, lam / n * dmean, rtol=1e-13, atol=0)
    np.testing.assert_allclose(dls_rows.sum(0), lam / n * dls, rtol=1e-13, atol=0)


def test_reference_adds_the_kl_part_to_the_policy_only():
    b = par.synthetic_batch(40, 1, 2)
    tpol, tmean, tstd = ks.teacher()
    tflat = ks.teacher_pdflat(tpol, tmean, tstd, b["z"])
    args = (b["pol"], b["vf"], b["z"], b["a"], b["lpo"], b["atarg"], b["ret"], 0.2)
    r0, r = par.reference(*args), ks.reference(*args, tflat, 0.7)
    np.testing.assert_array_equal(r["gvf"], r0["gvf"])
    np.testing.assert_array_equal(r["M_vf"], r0["M_vf"])
    np.testing.assert_array_equal(r["gpol_ppo"], r0["gpol"])
    np.testing.assert_array_equal(r["gpol"], r0["gpol"] + ks.kl_grad(b["pol"], b["z"], tflat, 0.7))
    assert np.all(r["M_pol"] >= np.abs(r["gpol"]) - 1e-15) and np.all(r["M_pol"] >= r0["M_pol"])
    np.testing.assert_array_equal(ks.reference(*args, tflat, 0.0)["gpol"], r0["gpol"])
