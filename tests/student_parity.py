"""Shared parity check of the two reference students' gradients (csrc/student_mlp*.h and
csrc/student_lstm*.h with rd_gemm.h) against oracle/refnet_np.py and oracle/lstm_np.py, in f32
and, against the emulations tests/refnet_bf16.py and tests/lstm_bf16.py, in the bf16 modes (test
infrastructure: imports oracle/ and those emulations, never the product).

Every gradient entry of either student is a sum over rows (MLP) or over windows x steps (LSTM) of
one dense product's terms a_in[r, i] dz[r, j], or of dz[r, j] alone for a bias.  As tests/parity.py
and tests/ppo_parity.py hold their gradients, each entry is held to the scale of that sum:

* global:    |g - g64| <= TOL_GLOBAL x max|g64|;
* per entry: |g - g64|_e <= TOL_ENTRY x M_e, with M_e = sum over the rows of |the row's contribution
  to e| = (|a_in|^T |dz|)_e for a kernel, (sum |dz|)_e for a bias; for the LSTM cell's Wl the sum
  over t of |[x_t, h_{t-1}]|^T |dz_t|, for Wp the sum over t of |prev_t|^T |dx_t[11:43]|;
* where M_e = 0 the entry is exactly 0 (under MSE the log-std columns of the last layer: 66 MLP
  entries, 66 per LSTM head).

dz is the oracle's signed backward (`mlp_products`, `lstm_products` walk it with the oracle's own
tanh_grad / cell_backward and dense_backward's products, and keep every product's operands; the
gradient they sum to is the oracle's to 1e-13, tests/test_student_parity_mutation.py).  Absolute values are taken of a
product's two operands only, never along the backward path: through five layers or ten BPTT steps
a backward on absolute values grows loose enough to hide a row.

bf16: `rounded` puts the rounded operands where the emulations round them (MLP layers 1-3: H and
dZ of the weight gradient, dZ and W of the data gradient; LSTM: [x_t | h_{t-1}] and dz_t of dWl,
dz_t and Wl of the data gradient; the biases sum the unrounded dz).  The comparison target is the
emulation's gradient, which these products sum to as well.

`row_contribution` is one row's (one window's) share of the gradient, on request restricted to
one product: the mutations of tests/test_student_parity_mutation.py and the oracle's side of the
GPU isolation tests.

Tolerances.  They start from tests/parity.py's pair and follow tests/ppo_parity.py's rule: every
GPU case is run once and its worst errors written to profiles/student_parity_errors.txt; a
tolerance stays while the worst measured error is at most a quarter of it, else it becomes 4 x the
worst measured error rounded up to one significant figure, and never more than the student's
TOL_CAP.  The caps are not measured on the GPU: each is half of the weakest mutation's per-entry
error that tests/test_student_parity_mutation.py computes at the largest shape the GPU tests use
(MLP 20,000 rows, kl: row 63 lost in layer 0's dW alone, 1.05e-4; LSTM (4, 2000), mse: one window's
t = 1 term of dWp, 3.56e-4); that test asserts both, and judges every mutation with the tolerances
in force.  Measured on MI355X (profiles/student_parity_errors.txt):

* MLP f32, 15 .. 20,000 rows: global <= 5.7e-7, per entry <= 1.8e-6: both tolerances stay.
* LSTM f32, 16 .. 2,000 windows: global <= 2.9e-7, per entry <= 2.2e-5 (mse, column 28 of head 2's
  W1 at every shape: 2.2e-5 at (10, 31), 1.8e-6 at (4, 2000)), so TOL_ENTRY_LSTM = 9e-5.  That
  column is no kernel error: dz1[:, 28] = (dz2 W2^T)[:, 28] cancels to 1 / 1,700 of its terms'
  magnitude (the median column: 1 / 11), and the same backward in numpy float32 on the oracle's
  activations misses the same entries by 2.5e-5.  M takes no absolute values along the path, so
  it does not cover the path's own conditioning; the tolerance does, and stays under the cap.
* One row (MLP n = 1) or one window (LSTM B = 1): an entry is a single term a_i dz_j, M_e = |it|
  and nothing averages the path's rounding: measured 5.4e-5 (MLP; numpy float32: 2.1e-5) and
  4.8e-4 (LSTM (3, 1)), more than the caps.  There the global bound and the exact zeros are
  asserted and the per-entry figure is only printed: a lost row of one is the whole gradient.
* bf16 against the emulations: an operand within an f32 ulp of a bf16 tie rounds the other way on
  the device, which moves that row's term by 2^-9 .. 2^-8 of itself, i.e. the entry by about
  2e-3 / rows of M_e: measured per entry 3e-7 .. 8e-6 at the shapes without such a flip (MLP n = 1,
  15, 16, 20, 63; LSTM (1, 7)) and 9e-5 .. 1.6e-3 at all others under 2,000 rows (MLP up to n = 330,
  LSTM up to (4, 330) with 1.4e-4 and (5, 40) with 1.5e-3; global up to 4.9e-5), 3.5e-5 at
  LSTM (4, 2000).  More than the caps, which stay: the bf16 bounds are asserted from
  BF16_MIN_ROWS = 2,000 rows per product on (LSTM (4, 2000): TOL_ENTRY_BF16 is 4 x 3.5e-5 = 2e-4
  cut to the cap), and below it only the exact zeros are, with the figures printed.  That hole
  is the size of one flip, not of the check: tests/test_student_parity_mutation.py shows that
  every mutation measures more than the cap at those shapes on the emulation's own products.
  The two sharded tests compare two device gradients of the same arithmetic and take the f32
  bounds (measured per entry <= 3.3e-7).

The isolation bound |d - d64|_e <= a x (M_e(x_r) + M_e(z)) + b x max(M_e(batch), M_e(batch with r
replaced)) has tests/parity.py's form and pair (1e-5, 5e-6) and follows the same rule: measured
worst error / bound 0.077 (MLP: stays), 0.33 (LSTM, 16 windows with the per-layer head): the
LSTM's pair becomes (2e-5, 1e-5).
"""
from typing import NamedTuple, Optional

import numpy as np

from oracle import lstm_np as ln
from oracle import policy_np as pn
from oracle import refnet_np as rn
from oracle.refnet_np import tanh_grad

TOL_GLOBAL = 1e-5            # x max|g64|, f32 modes (measured <= 5.7e-7)
TOL_ENTRY_MLP = 2e-5         # x M_e, f32 (measured <= 1.8e-6 from 15 rows on)
TOL_ENTRY_LSTM = 9e-5        # x M_e, f32 (measured <= 2.2e-5 from 16 windows on)
TOL_GLOBAL_BF16 = 1e-5       # bf16 modes against the emulation, from BF16_MIN_ROWS rows on (measured 9.4e-7)
TOL_ENTRY_BF16 = 1.7e-4      # (measured 3.5e-5 at LSTM (4, 2000): 4 x that, cut to the cap)
BF16_MIN_ROWS = 2000         # rows per product (MLP rows, LSTM windows) from which the bf16 bounds are asserted
TOL_CAP_MLP = 5.2e-5         # half of 1.05e-4: one row of 20,000 lost in layer 0's dW
TOL_CAP_LSTM = 1.7e-4        # half of 3.56e-4: one window of (4, 2000) lost in dWp at one step
ISO_MLP = (1e-5, 5e-6)       # the isolation bound's a x (M(x_r) + M(z)) + b x max(M(batch), M(batch with r replaced))
ISO_LSTM = (2e-5, 1e-5)


class Product(NamedTuple):
    """One dense product of the backward: block += a^T dz, bias += sum over rows of dzb."""
    block: str
    bias: str
    a: np.ndarray             # [rows, in]   as the weight gradient reads it
    dz: np.ndarray            # [rows, out]  as the weight gradient reads it
    dzb: np.ndarray           # [rows, out]  as the bias gradient sums it
    t: Optional[int]          # the LSTM's unrolled step; None for the MLP


def _r(a, on):
    return pn.bf16(a) if on else a


# ---------------------------------------------------------------- layouts
def mlp_layout():
    """name -> (offset, shape): W0, b0 .. W4, b4 (layer 0 is the input layer 16 -> 24)."""
    out = {}
    for li, (w, bo, a, b) in enumerate(rn.LAYOUT):
        out[f"W{li}"] = (w, (a, b))
        out[f"b{li}"] = (bo, (b,))
    return out, rn.P_REF


def lstm_layout(T):
    """oracle/lstm_np.layout: Wp, bp, Wl, bl, h{t}/W{k}, h{t}/b{k}."""
    return ln.layout(T)


def _layout_of(size):
    if size == rn.P_REF:
        return mlp_layout()
    return lstm_layout(ln.steps_of(np.empty(size)))


def block_of(layout, k):
    """(name, index within the block) of flat entry k."""
    for name, (o, s) in layout.items():
        n = int(np.prod(s))
        if o <= k < o + n:
            return name, tuple(int(i) for i in np.unravel_index(k - o, s))
    raise IndexError(k)


def block_slice(layout, name):
    o, s = layout[name]
    return slice(o, o + int(np.prod(s)))


# ---------------------------------------------------------------- the backward's products
def mlp_products(p, fw, dout, rounded=()):
    """The five products of refnet_np.backward (rounded=()) or of refnet_bf16.backward (rounded=
    refnet_bf16.BF_LAYERS) on the forward fw of the same `rounded`, rows = the batch's rows."""
    Ws = rn.unpack(np.asarray(p, np.float64))
    hs = fw["hs"]
    out, dz = [], np.asarray(dout, np.float64)
    for li in range(len(Ws) - 1, -1, -1):
        on = li in rounded
        a, dzr = _r(hs[li], on), _r(dz, on)
        out.append(Product(f"W{li}", f"b{li}", a, dzr, dz, None))
        if li > 0:
            dh = dzr @ _r(Ws[li][0], on).T               # dense_backward's da_in
            dz = tanh_grad(hs[li], dh) if rn.ACT[li - 1] else dh
    return out


def lstm_products(p, fw, dout, rounded=False):
    """The products of lstm_np.backward (rounded=False) or lstm_bf16.backward (True) on the forward
    fw of the same `rounded`, rows = the windows: per step five head layers, the cell matrix and
    the prev_pdflat projection."""
    W = ln.unpack(p)
    C = fw["cache"]
    T = len(C["x"])
    out, dh_out = [], []
    for t in range(T):
        a = C["acts"][t]
        dz = np.asarray(dout[t], np.float64)
        for k in range(5, 0, -1):
            out.append(Product(f"h{t}/W{k}", f"h{t}/b{k}", a[k - 1], dz, dz, t))
            da = dz @ W[f"h{t}/W{k}"].T
            if k > 1:
                dz = tanh_grad(a[k - 1], da)
        dh_out.append(da)
    WlT = _r(W["Wl"], rounded).T
    dh_next = np.zeros_like(np.asarray(C["hprev"][-1], np.float64))
    dc_next = np.zeros_like(dh_next)
    for t in range(T - 1, -1, -1):
        s = dict(gi=C["gi"][t], gj=C["gj"][t], gf=C["gf"][t], go=C["go"][t], c=C["c"][t], cprev=C["cprev"][t])
        dz, dc_next = ln.cell_backward(s, dh_out[t] + dh_next, dc_next)
        xin = np.concatenate([C["x"][t], C["hprev"][t]], 1)
        dzr = _r(dz, rounded)
        out.append(Product("Wl", "bl", _r(xin, rounded), dzr, dz, t))
        dxin = dzr @ WlT
        dh_next = dxin[:, ln.IN_X:]
        dp = dxin[:, 11:ln.IN_X]
        out.append(Product("Wp", "bp", np.asarray(fw["prev"][t], np.float64), dp, dp, t))
    return out


def _sum(products, layout, size, rows=None, only=None, absolute=False):
    """The flat vector the products sum to, over `rows` (all), with absolute operands on request;
    `only` = a kernel block's name or (name, t): that one product's dW alone (no bias)."""
    out = np.zeros(size)
    want = (only, None) if isinstance(only, str) else only
    for pr in products:
        if want is not None and (pr.block != want[0] or (want[1] is not None and pr.t != want[1])):
            continue
        a, dz, dzb = (pr.a, pr.dz, pr.dzb) if rows is None else (pr.a[rows], pr.dz[rows], pr.dzb[rows])
        if absolute:
            a, dz, dzb = np.abs(a), np.abs(dz), np.abs(dzb)
        out[block_slice(layout, pr.block)] += (a.T @ dz).ravel()
        if want is None:
            out[block_slice(layout, pr.bias)] += dzb.sum(0)
    return out


def gradient(products, size):
    """The gradient the products sum to: the oracle's (or the emulation's) backward."""
    return _sum(products, _layout_of(size)[0], size)


def scale(products, size, rows=None):
    """M: per entry the sum over the rows of |the row's contribution|."""
    return _sum(products, _layout_of(size)[0], size, rows=rows, absolute=True)


def row_contribution(products, size, rows, only=None):
    """The contribution of `rows` (MLP: batch rows; LSTM: windows, over every step) to the gradient;
    only = "W2" or ("Wl", 3) or ("h2/W3", None): restricted to that product's dW."""
    return _sum(products, _layout_of(size)[0], size, rows=np.atleast_1d(rows), only=only)


def mlp_scale(p, fw, dout, rounded=()):
    return scale(mlp_products(p, fw, dout, rounded), rn.P_REF)


def lstm_scale(p, fw, dout, rounded=False):
    return scale(lstm_products(p, fw, dout, rounded), np.asarray(p).size)


# ---------------------------------------------------------------- references, computed once per case
def mlp_reference(p, x, t, loss, n_global=None, rounded=(), **drop):
    """dict(g64, M, products, loss, sq) of one MLP training launch on rows x (after input dropout
    `drop` = keep_prob, seed, step, row_base); rounded=refnet_bf16.BF_LAYERS: the emulation's."""
    from tests import refnet_bf16 as rb
    xd = rn.dropout(x, drop.get("keep_prob", 1.0), seed=drop.get("seed", 0), step=drop.get("step", 0),
                    row_base=drop.get("row_base", 0))
    fw = rb.forward(p, xd, rounded)
    lval, d, sq = rn.loss_and_dout(fw["pdflat"], t, loss, n_global or len(x))
    pr = mlp_products(p, fw, d, rounded)
    return dict(g64=gradient(pr, rn.P_REF), M=scale(pr, rn.P_REF), products=pr, loss=lval, sq=sq, size=rn.P_REF)


def lstm_reference(p, ob, prev, t, loss, state0=None, windows_global=None, rounded=False, **drop):
    """The same for one LSTM rollout over windows ob, prev, t [T, B, .]."""
    from tests import lstm_bf16 as lb
    T, B, _ = np.asarray(ob).shape
    obd = ln.dropout(ob, drop.get("keep_prob", 1.0), drop.get("seed", 0), drop.get("step", 0), drop.get("row_base", 0))
    fw = lb.forward(p, obd, prev, state0, rounded)
    lval, d, sq = ln.loss_and_dout(fw["pdflat"], t, loss, T * (windows_global or B))
    pr = lstm_products(p, fw, d, rounded)
    size = np.asarray(p).size
    return dict(g64=gradient(pr, size), M=scale(pr, size), products=pr, loss=lval, sq=sq, size=size, fw=fw)


# ---------------------------------------------------------------- report and verdict
def grad_report(g, g64, M):
    """Errors of a kernel gradient g against g64 with scale M: global (x max|g64|), per entry
    (x M_e; entries with M_e = 0 must be exactly 0), the worst entry, its block and its index
    within the block (row = input unit, column = output unit)."""
    g = np.asarray(g, np.float64)
    d = np.abs(g - g64)
    glob = float(d.max() / max(np.abs(g64).max(), 1e-300))
    zero = M == 0
    ent = np.where(zero, np.where(d > 0, np.inf, 0.0), d / np.where(zero, 1.0, M))
    k = int(np.argmax(ent))
    blk, idx = block_of(_layout_of(g.size)[0], k)
    return {"global": glob, "entry": float(ent[k]), "worst_entry": k, "block": blk, "index": idx, "zeros": int(zero.sum())}


def _is_mlp(size):
    return size == rn.P_REF


def tolerances(size, bf16=False):
    """(tol_entry, tol_global, cap) for a gradient of `size` floats."""
    cap = TOL_CAP_MLP if _is_mlp(size) else TOL_CAP_LSTM
    if bf16:
        return min(TOL_ENTRY_BF16, cap), TOL_GLOBAL_BF16, cap
    return (TOL_ENTRY_MLP if _is_mlp(size) else TOL_ENTRY_LSTM), TOL_GLOBAL, cap


def in_force(rows, bf16=False):
    """(per-entry bound asserted, global bound asserted) for a batch of `rows` rows per product
    (MLP rows, LSTM windows): see "Tolerances" above.  The exact zeros are asserted always."""
    if bf16:
        return rows >= BF16_MIN_ROWS, rows >= BF16_MIN_ROWS
    return rows > 1, True


def grad_ok(g, g64, M, rows, bf16=False):
    """The verdict in force for `rows` rows per product, and the report."""
    r = grad_report(g, g64, M)
    te, tg, _ = tolerances(np.asarray(g).size, bf16)
    entry, glob = in_force(rows, bf16)
    exact = bool((np.asarray(g, np.float64)[M == 0] == g64[M == 0]).all())
    r["asserted"] = "entry global" if entry else "global, zeros" if glob else "zeros"
    return exact and (not glob or r["global"] <= tg) and (not entry or r["entry"] <= te), r


def check_grad(g, ref, label, rows, bf16=False):
    """Assert a kernel gradient against a reference dict (g64, M), after printing the report line
    (profiles/student_parity_errors.txt is made of these lines)."""
    ok, r = grad_ok(g, ref["g64"], ref["M"], rows, bf16)
    print(f"student_parity {label}: global {r['global']:.2e} entry {r['entry']:.2e} ({r['block']}{list(r['index'])}) "
          f"zero entries {r['zeros']} asserted: {r['asserted']}")
    assert ok, (label, r)
    return r


# ---------------------------------------------------------------- per-row isolation
def isolation_bound(M_x, M_z, M_all, M_r):
    """tests/parity.py's form: a x (M(x_r) + M(z)) + b x max(M(batch), M(batch with r replaced));
    a single row's M is scale(products, size, rows=[r])."""
    a, b = ISO_MLP if _is_mlp(M_all.size) else ISO_LSTM
    return a * (M_x + M_z) + b * np.maximum(M_all, M_r)


def isolation_ratio(d, d64, bound):
    """max over entries of |d - d64| / bound (inf where the bound is 0 and the error is not), and
    the entry."""
    err = np.abs(np.asarray(d, np.float64) - d64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    k = int(np.argmax(r))
    return float(r[k]), k


# the fixed replacement row / window of the isolation tests (GPU and CPU)
ISO_MLP_Z = (np.linspace(-.6, .7, 16).astype(np.float32), np.array([.2, -.1, -.5, -.7], np.float32))


def iso_lstm_z(T):
    """(ob [T,11], prev [T,4], target [T,4]) of the replacement window."""
    from tests import lstm_bf16 as lb
    ob, prev, t = lb.batch(T, 1, 0)
    return ob[:, 0], prev[:, 0], t[:, 0]


# ---------------------------------------------------------------- bf16 batches without an operand on a tie
TIE_ULPS = 8                 # f32 ulps; the device's f32 sums and tanhf move an activation by about one
TIE_MAX_ROWS = 20            # up to here one flipped row can exceed the files' relative L2 bound of 2e-4


def mlp_bf16_tie_distance(p, x):
    """The smallest distance, in f32 ulps, of a forward operand of the bf16 layers (the emulation's
    activations h1 .. h3 as f32) to a bf16 rounding tie, where the device may round the other way."""
    from tests import refnet_bf16 as rb
    hs = rb.forward(p, x)["hs"]
    low = np.concatenate([(hs[li].astype(np.float32).view(np.uint32) & 0xFFFF).ravel() for li in rb.BF_LAYERS])
    return int(np.abs(low.astype(np.int64) - 0x8000).min())


def mlp_bf16_seed(n, first):
    """The batch seed of a bf16 MLP case of n <= TIE_MAX_ROWS rows: the first seed from `first` on
    whose refnet_bf16.batch has no forward operand within TIE_ULPS of a tie.  (n = 15 from seed 22
    has one exactly on a tie, layer 2's input [3, 26]; rounding it the other way moves the mse
    gradient by 3.1e-4 in relative L2, which is what an MI355X measured: 3.13e-4.)  The rule reads
    the emulation alone."""
    from tests import refnet_bf16 as rb
    assert n <= TIE_MAX_ROWS
    seed = first
    while mlp_bf16_tie_distance(rb.params(), rb.batch(n, seed)[0]) <= TIE_ULPS:
        seed += 1
    return seed
