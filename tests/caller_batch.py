"""Shared inputs and oracle references of the caller-batch (obs / rows mode) tests: the layout
table of tests/test_caller_batch_gpu.py, the nets (non-zero biases, non-trivial observation
filters, a non-zero student log-std), the observation rows with their recorded teacher pdflat,
and the f64 oracle gradient of either mode with every row's own contribution (test
infrastructure: imports oracle/, never the product path)."""
import functools
import os
import re

import numpy as np

from oracle import policy_np as pn
from tests import parity
from tests.conftest import ROOT

GRID = 2   # DistillConfig(grid=2): ws_rows = 2, so 2 x PAIRS = 8 pairs in total
# n -> (obs mode with the f32 student, rows mode), each (rows per group, workgroups, helper-pair kernel).
# The bf16 student never takes the helper kernel: its obs mode has the rows-mode layout.
LAYOUTS = {
    1: ((16, 1, True), (16, 1, False)),      # one row; 15 idle lanes in the only tile
    17: ((16, 1, True), (16, 1, False)),     # ragged second group (1 row)
    33: ((16, 2, True), (16, 1, False)),     # helper: workgroup 1 has one owner and one idle helper
    64: ((16, 2, True), (16, 1, False)),     # the last n at which the helper layout holds
    65: ((16, 2, False), (16, 2, False)),    # first n past the helper cap
    203: ((16, 2, False), (16, 2, False)),   # 13 groups on 8 pairs; last tile has 11 rows
    257: ((32, 2, False), (32, 2, False)),   # 9 groups; the last holds one row
    499: ((32, 2, False), (32, 2, False)),   # two groups per pair; last group 19 rows = 2 tiles, the second with 3
    513: ((64, 2, False), (64, 2, False)),   # 9 groups; the last holds one row (ntile = 1 of 4)
    1000: ((64, 2, False), (64, 2, False)),  # two groups per pair; last group 40 rows = 3 tiles, the third with 8
}
TAIL = 64   # rows of padding behind the n rows of a device buffer (NaN: a consumed one poisons the gradient)


def layout_constants():
    """WAVES, GROUP and TILE of csrc/distill_layout.h, which the table above is derived from:
    8 pairs at grid = 2, helper layout up to 2 x 2 sixteen-row groups = 64 rows, 32-row groups
    from 32 x 8 = 256 rows, 64-row groups from 64 x 8 = 512 rows."""
    txt = open(os.path.join(ROOT, "reacherdistilation_amd", "csrc", "distill_layout.h")).read()
    return {k: int(re.search(r"\b" + k + r" = (\d+)[,;]", txt).group(1)) for k in ("WAVES", "GROUP", "TILE")}


@functools.lru_cache(maxsize=None)
def nets():
    """(teacher, student) with every bias, both observation filters and the student's log-std
    non-trivial, so that a lost bias or filter term shows."""
    from reacherdistilation_amd.policy import student_init, synthetic_teacher
    t, s = synthetic_teacher(1), student_init(2)
    rs = np.random.RandomState(123)
    for p in (t, s):
        p.ob_mean = rs.uniform(-.1, .1, 11).astype(np.float32)
        p.ob_std = rs.uniform(.5, 2, 11).astype(np.float32)
        p.ob_std[6:8] = rs.uniform(.6, .9, 2)   # the velocity inputs (rows(): up to +-5) pass the clip at +-5 std
        p.flat[pn.P_B1:pn.P_W2] = rs.uniform(-.2, .2, 64)
        p.flat[pn.P_B2:pn.P_W3] = rs.uniform(-.2, .2, 64)
        p.flat[pn.P_B3:pn.P_LS] = rs.uniform(-.1, .1, 2)
    s.flat[pn.P_LS:pn.P_TOT] = (-0.2, 0.1)
    return t, s


def rows(n, seed):
    """n observation rows (f32; the velocity columns reach +-5, past both filters' clip) and their
    recorded teacher pdflat (mean | log-std per row in [-3.5, -0.5]), as tests/test_rows_gpu.py."""
    rs = np.random.RandomState(seed)
    q0, q1 = rs.uniform(-3, 3, n), rs.uniform(-3, 3, n)
    ob = np.stack([np.cos(q0), np.cos(q1), np.sin(q0), np.sin(q1), rs.uniform(-.2, .2, n), rs.uniform(-.2, .2, n),
                   rs.uniform(-5, 5, n), rs.uniform(-5, 5, n), rs.uniform(-.3, .3, n), rs.uniform(-.3, .3, n),
                   np.zeros(n)], 1).astype(np.float32)
    t = np.concatenate([rs.uniform(-.5, .5, (n, 2)), rs.uniform(-3.5, -0.5, (n, 2))], 1).astype(np.float32)
    return ob, t


# A batch of ONE row turns the per-entry bound TOL_ENTRY x M_e into a relative bound on single
# products of that row: dW3_j = h2_j dmean, dW2_kj = h1_k dZ2_j, dZ = (...)(1 - h^2).  The f32
# arithmetic the kernel is specified to use limits what one row resolves there, whatever the
# kernel does: tanh as 1 - 2 / (2^y + 1) (rd_device.h) is exact to an ulp or two of 1, not of h,
# so a unit near 0 or near saturation loses relative precision in h or in 1 - h^2, and a
# pre-activation formed by cancellation does the same (csrc/distill_forward.h: the f32 and the
# split products are exact to 1.3e-7 / 1.5e-7 of sum|terms|); M_e, the oracle's backward on
# absolute values, shrinks with these factors.  From a few rows up the other rows' terms carry M_e.
# single_row_error_bound() propagates those two figures to first order, every error at its
# maximum and with the worst sign, through the forward and backward of one row.  Over the
# 64-term chains the errors add like a random walk, sqrt(64) = 8 below that worst case, so a row
# whose bound is within SINGLE_ROW_BOUND = 5 x TOL_ENTRY x M_e is expected near half of the
# tolerance; a typical row's bound is 30 x (one row in twenty within 8 x).  The single row of the
# n = 1 cases is the first seed within it, in both modes and losses; chosen on the CPU alone.
# Measured on MI355X afterwards: <= 4.1e-6 x M_e at that row (profiles/caller_batch_parity.txt);
# rows taken without the rule gave 1.4e-4 (seed 1: a saturated unit, 1 - h^2 ~ 2e-3), 3.3e-5
# (seed 2) and 2.2e-5 (seed 24: h2 ~ 0.004 from a cancelled pre-activation), global <= 6e-7 each.
SINGLE_ROW_BOUND = 5.0
SINGLE_ROW_SEED = 246   # tests/test_parity_mutation.py re-checks the rule
PRODUCT_ERR, TANH_ERR, ULP = 1.5e-7, 2.0 ** -23, 2.0 ** -24


def _forward_error(p, ob):
    q = pn.unpack(p.flat.astype(np.float64))
    f = pn.forward(p.flat.astype(np.float64), p.ob_mean.astype(np.float64), p.ob_std.astype(np.float64),
                   ob.astype(np.float64))
    z, h1, h2 = f["z"][0], f["h1"][0], f["h2"][0]
    W2, W3 = np.abs(q["W2"]), np.abs(q["W3"])
    e_h1 = (1 - h1 ** 2) * (PRODUCT_ERR + 2 * ULP) * (np.abs(z) @ np.abs(q["W1"]) + np.abs(q["b1"])) + TANH_ERR
    e_h2 = (1 - h2 ** 2) * (PRODUCT_ERR * (np.abs(h1) @ W2 + np.abs(q["b2"])) + e_h1 @ W2) + TANH_ERR
    e_mean = PRODUCT_ERR * (np.abs(h2) @ W3 + np.abs(q["b3"])) + e_h2 @ W3
    return q, f, e_h1, e_h2, e_mean


def single_row_error_bound(mode, seed, loss):
    """The worst-case first-order f32 error of the gradient of rows(1, seed), per entry, as a
    multiple of TOL_ENTRY x M_e (its largest entry)."""
    return row_error_bound(mode, *rows(1, seed), loss)


def row_error_bound(mode, ob, t, loss):
    """single_row_error_bound() of a given row: observation ob [1, 11] and, in rows mode, its
    recorded pdflat t [1, 4]."""
    e, M = row_error_terms(mode, ob, t, loss)
    return float((e[M > 0] / M[M > 0]).max() / parity.TOL_ENTRY)


def row_error_terms(mode, ob, t, loss):
    """(e, M) of row_error_bound(): the first-order error bound and the scale M_e per gradient
    entry, both at n_global = 1 (rows of one launch add in each)."""
    teacher, student = nets()
    q, f, e_h1, e_h2, e_ms = _forward_error(student, ob)
    z, h1, h2 = f["z"][0], f["h1"][0], f["h2"][0]
    if mode == "obs":
        _, ft, _, _, e_mt = _forward_error(teacher, ob)
        mt, lt = ft["mean"][0], teacher.flat[pn.P_LS:].astype(np.float64)
    else:
        e_mt, mt, lt = 0.0, t[0, :2].astype(np.float64), t[0, 2:].astype(np.float64)
    d = f["mean"][0] - mt
    e_d = e_ms + e_mt + ULP * np.abs(d)
    if loss == "mse":
        dm, e_dm, e_ls = d, e_d + 2 * ULP * np.abs(d), np.zeros(2)
    else:   # 1 / var_t and var_s through __expf: 1e-6 relative
        rr = np.exp(-2 * lt)
        dm, e_dm, e_ls = d * rr, e_d * rr + 1e-6 * np.abs(d * rr), 2e-6 * np.exp(2 * f["logstd"]) * rr
    W2, W3 = np.abs(q["W2"]), np.abs(q["W3"])
    s1, s2 = 1 - h1 ** 2, 1 - h2 ** 2
    e_W3 = np.outer(e_h2, np.abs(dm)) + np.outer(np.abs(h2), e_dm)
    g2 = q["W3"] @ dm
    e_dz2 = (W3 @ e_dm + 2 * ULP * (W3 @ np.abs(dm))) * s2 + np.abs(g2) * 2 * np.abs(h2) * e_h2
    dz2 = g2 * s2
    e_W2 = np.outer(e_h1, np.abs(dz2)) + np.outer(np.abs(h1), e_dz2)
    dh1 = q["W2"] @ dz2
    e_dz1 = (PRODUCT_ERR * (W2 @ np.abs(dz2)) + W2 @ e_dz2) * s1 + np.abs(dh1) * 2 * np.abs(h1) * e_h1
    e_W1 = np.outer(np.abs(z), e_dz1 + 2 * ULP * np.abs(dh1 * s1))
    e = pn.pack(e_W1, e_dz1, e_W2, e_dz2, e_W3, e_dm, e_ls)
    return e, oracle(mode, ob, t, loss, 1)[1]


def single_row_ok(seed):
    return all(single_row_error_bound(mode, seed, loss) <= SINGLE_ROW_BOUND
               for mode in ("obs", "rows") for loss in ("mse", "kl"))


@functools.lru_cache(maxsize=None)
def batch(n, seed=None):
    """The rows of the size-n cases (seed n unless given; n = 1: SINGLE_ROW_SEED); read-only."""
    if seed is None:
        seed = SINGLE_ROW_SEED if n == 1 else n
    ob, t = rows(n, seed)
    ob.setflags(write=False)
    t.setflags(write=False)
    return ob, t


def clipped(ob, p):
    """How many filtered inputs of net p the clip to +-5 catches."""
    z = (ob.astype(np.float64) - p.ob_mean) / p.ob_std
    return int((np.abs(z) > pn.OB_CLIP).sum())


def oracle(mode, ob, t, loss, n_global, bf16=False, sp=None):
    """(g64, M, loss, sq) of one caller batch in f64: mode "obs" relabels ob with the teacher of
    nets(), mode "rows" takes the recorded t; sp: the student's parameters (nets()'s own if None)."""
    teacher, student = nets()
    sp = student.flat if sp is None else sp
    ob64 = ob.astype(np.float64)
    if mode == "rows":
        return parity.oracle_grad_rows(sp, student, ob64, t, loss, n_global, bf16=bf16)
    g64, M, (fs, ft, L, sq) = parity.oracle_grad(sp, teacher, student, ob64, loss, n_global, bf16=bf16)
    return g64, M, L, sq


@functools.lru_cache(maxsize=None)
def reference(mode, n, loss, bf16=False, seed=None):
    """oracle() of batch(n, seed), computed once per case and shared; read-only."""
    ob, t = batch(n, seed)
    g64, M, L, sq = oracle(mode, ob, t, loss, n, bf16)
    g64.setflags(write=False)
    M.setflags(write=False)
    return g64, M, L, sq


def row_contributions(mode, ob, t, loss, n_global, sel):
    """The summed contribution of rows `sel` to the f32 student's oracle gradient (the log-std
    entries included: each row adds its own var_s / var_t - 1 under KL)."""
    teacher, student = nets()
    sp = student.flat.astype(np.float64)
    ob64 = ob.astype(np.float64)
    fs = pn.forward(sp, student.ob_mean.astype(np.float64), student.ob_std.astype(np.float64), ob64)
    if mode == "rows":
        _, dmean, _, _, _ = parity.loss_rows(fs, t, loss, n_global)
        lt = t[:, 2:].astype(np.float64)
    else:
        ft = pn.forward(teacher.flat.astype(np.float64), teacher.ob_mean.astype(np.float64),
                        teacher.ob_std.astype(np.float64), ob64)
        _, dmean, _, _ = pn.loss_and_dmean(fs, ft, loss, n_global)
        lt = np.broadcast_to(ft["logstd"], (ob.shape[0], 2))
    sel = np.asarray(sel)
    dls = (np.exp(2 * fs["logstd"]) / np.exp(2 * lt[sel]) - 1.0).sum(0) if loss == "kl" else np.zeros(2)
    f = {k: (v[sel] if getattr(v, "ndim", 0) == 2 else v) for k, v in fs.items()}
    return pn.backward(sp, f, dmean[sel], dls)


# ---------------------------------------------------------------- the bf16 student as a kernel forms it
# (f32 accumulation and the kernels' f32 tanh in place of the bf16 oracle's f64: the stand-in that
# tells whether a batch leaves room for flipped bf16 roundings; tests/test_caller_batch_gpu.py,
# tests/env_batch.py)
def tanh_f32(pre):
    """tanh as the kernels form it (rd_device.h tanh_pre), every step rounded to f32:
    1 - 2 / (2^y + 1), y = 2 log2(e) pre."""
    f32 = np.float32
    y = (pre * f32(2.8853900817779268)).astype(f32)
    e = np.exp2(y.astype(np.float64)).astype(f32)
    r = (1.0 / (e + f32(1)).astype(f32).astype(np.float64)).astype(f32)
    return (1.0 - 2.0 * r.astype(np.float64)).astype(f32).astype(np.float64)


def forward_bf16_f32_accumulation(p, obmu, obsd, ob):
    """pn.forward_bf16 with the two hidden layers' pre-activations accumulated in f32 (numpy's f32
    matmul) and their tanh formed in f32, as a kernel does, instead of f64."""
    q = pn.unpack(np.asarray(p, np.float64))
    f32 = np.float32
    rs = (f32(1) / np.asarray(obsd, f32)).astype(f32)
    z = np.clip((np.asarray(ob, f32) - np.asarray(obmu, f32)) * rs, f32(-5), f32(5)).astype(f32)
    zb = pn.bf16(z)
    h1 = tanh_f32(zb.astype(f32) @ pn.bf16(q["W1"]).astype(f32) + q["b1"].astype(f32))
    h2 = tanh_f32(pn.bf16(h1).astype(f32) @ pn.bf16(q["W2"]).astype(f32) + q["b2"].astype(f32))
    return dict(z=z.astype(np.float64), zb=zb, h1=h1, h2=h2, mean=h2 @ pn.bf16(q["W3"]) + q["b3"], logstd=q["ls"])


def teacher_mean_f32(p, ob):
    """The f32 teacher's mean with every layer formed in f32."""
    f32 = np.float32
    q = {k: v.astype(f32) for k, v in pn.unpack(p.flat).items()}
    z = np.clip((np.asarray(ob, f32) - p.ob_mean) * (f32(1) / p.ob_std).astype(f32), f32(-5), f32(5)).astype(f32)
    h1 = tanh_f32(z @ q["W1"] + q["b1"]).astype(f32)
    h2 = tanh_f32(h1 @ q["W2"] + q["b2"]).astype(f32)
    return (h2 @ q["W3"] + q["b3"]).astype(f32)
