"""The closed-loop query of the LSTM student on its bf16 cell (rdl_set_query_dtype's RDL_DTYPE_BF16,
include/reacher_student_lstm.h "Arithmetic"), restated over a whole chain of queries: siblings of
tests/test_student_lstm_evaluate_gpu.py's _oracle_chain on tests/lstm_bf16.py's emulation (rounded
operands, f64 sums), and an f32 stand-in of the device for the host-side check of the bounds.

A query is one forward over the window of the episode's last T records, rebuilt here from the
records themselves (ob | the previous record's t_pdflat; zero rows before the episode's first), from
the (c, h) the query before left -- chained inside the restatement, over the resets too.
"""
import numpy as np

from oracle import lstm_np as ln
from oracle import policy_np as pn
from tests import lstm_bf16 as lb

STEPS = 50
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20


def windows(rec, e, s, T):
    """(ob_w [T, n, 11], prev_w [T, n, 4]) of episode e's query s, from records [E, n, 50, 21]."""
    n = rec.shape[1]
    ob_w, prev_w = np.zeros((T, n, 11)), np.zeros((T, n, 4))
    for p in range(T):
        j = s - (T - 1) + p
        if j >= 0:
            ob_w[p] = rec[e, :, j, :F_REW]
            if j > 0:
                prev_w[p] = rec[e, :, j - 1, F_T:F_S]
    return ob_w, prev_w


def emulation_chain(rec, params, T, rounded=True, forward=lb.forward):
    """_oracle_chain on tests.lstm_bf16.forward: position T-1's pdflat of every query, [E, n, 50, 4],
    the state chained in the emulation.  rounded=False is _oracle_chain itself."""
    E, n = rec.shape[:2]
    want = np.zeros((E, n, STEPS, 4))
    state = None
    for e in range(E):
        for s in range(STEPS):
            ob_w, prev_w = windows(rec, e, s, T)
            fw = forward(params, ob_w, prev_w, state, rounded)
            state = fw["state"]
            want[e, :, s] = fw["pdflat"][T - 1]
    return want


def forward_f32(p, ob, prev, state0=None, rounded=True):
    """A stand-in for the device: tests.lstm_bf16.forward's operations with every value and every sum
    in f32 (numpy's own summation order and exp / tanh), head T-1 only.  Not the device's bits: it
    shows what f32 sums and the roundings they flip cost against the f64 emulation."""
    f = np.float32
    W = {k: v.astype(f) for k, v in ln.unpack(p).items()}
    T, B, _ = ob.shape
    c = np.zeros((B, ln.UNITS), f) if state0 is None else np.asarray(state0[0], f)
    h = np.zeros((B, ln.UNITS), f) if state0 is None else np.asarray(state0[1], f)
    r = (lambda a: pn.bf16(a).astype(f)) if rounded else (lambda a: a)
    Wl = r(W["Wl"])
    for t in range(T):
        x = np.concatenate([ob[t].astype(f), prev[t].astype(f) @ W["Wp"] + W["bp"]], 1)
        z = r(np.concatenate([x, h], 1)) @ Wl + W["bl"]
        i, j, g, o = np.split(z, 4, axis=1)
        sig = lambda v: f(1.0) / (f(1.0) + np.exp(-v))
        c = sig(g + f(ln.FORGET_BIAS)) * c + sig(i) * np.tanh(j)
        h = sig(o) * np.tanh(c)
    a = h
    for k in range(1, 5):
        a = np.tanh(a @ W[f"h{T - 1}/W{k}"] + W[f"h{T - 1}/b{k}"])
    y = np.zeros((T, B, 4), f)
    y[T - 1] = a @ W[f"h{T - 1}/W5"] + W[f"h{T - 1}/b5"]
    assert y.dtype == f and c.dtype == f and h.dtype == f
    return dict(pdflat=y, state=(c, h))


def bounds(got, emu, ora):
    """(median |got - emu|, max |got - emu|, cap = max |emu - ora|): the forward test's two quantities
    and the cap of the second (tests/test_student_lstm_bf16_gpu.py "Bounds")."""
    err = np.abs(np.asarray(got, np.float64) - emu)
    return float(np.median(err)), float(err.max()), float(np.abs(emu - ora).max())
