"""The bf16 mixed-precision arithmetic of the LSTM student (rdl_create_dtype's RDL_DTYPE_BF16,
include/reacher_student_lstm.h "Arithmetic"), restated on the oracle's building blocks
(oracle/lstm_np.py, oracle/policy_np.bf16) with f64 sums.

With ``rounded`` the three products of the cell matrix round their operands to bf16
(round-to-nearest-even): [x_t | h_{t-1}] and Wl in the forward, dz_t and Wl in the data gradient,
[x_t | h_{t-1}] and dz_t in the weight gradient.  The biases, the prev_pdflat projection, the gate
nonlinearities, c, h, the cell's backward point-wise arithmetic (on the unrounded stored gates and
c), the heads, the loss, dbl (the unrounded dz summed), dWp and dbp are exact.  With
``rounded=False`` this is lstm_np.forward / backward, operation for operation.
"""
import numpy as np

from oracle import lstm_np as ln
from oracle import policy_np as pn
from oracle.refnet_np import dense_backward, tanh_grad


def _r(a, on):
    return pn.bf16(a) if on else a


def forward(p, ob, prev, state0=None, rounded=True):
    """lstm_np.forward's result (pdflat [T,B,4], state, cache) with the gate product's operands rounded."""
    W = ln.unpack(p)
    ob = np.asarray(ob, np.float64)
    prev = np.asarray(prev, np.float64)
    T, B, _ = ob.shape
    c = np.zeros((B, ln.UNITS)) if state0 is None else np.asarray(state0[0], np.float64)
    h = np.zeros((B, ln.UNITS)) if state0 is None else np.asarray(state0[1], np.float64)
    Wl = _r(W["Wl"], rounded)
    cache = dict(x=[], hprev=[], cprev=[], gi=[], gj=[], gf=[], go=[], c=[], h=[], acts=[])
    ys = []
    for t in range(T):
        pt = prev[t] @ W["Wp"] + W["bp"]
        x = np.concatenate([ob[t], pt], 1)
        cache["x"].append(x); cache["hprev"].append(h); cache["cprev"].append(c)
        z = _r(np.concatenate([x, h], 1), rounded) @ Wl + W["bl"]
        i, j, f, o = np.split(z, 4, axis=1)
        gi, gj, gf, go = ln.sig(i), np.tanh(j), ln.sig(f + ln.FORGET_BIAS), ln.sig(o)
        c = gf * c + gi * gj
        h = go * np.tanh(c)
        for k, v in (("gi", gi), ("gj", gj), ("gf", gf), ("go", go), ("c", c), ("h", h)):
            cache[k].append(v)
        a = [h]
        for k in range(1, 5):
            a.append(np.tanh(a[-1] @ W[f"h{t}/W{k}"] + W[f"h{t}/b{k}"]))
        ys.append(a[-1] @ W[f"h{t}/W5"] + W[f"h{t}/b5"])
        cache["acts"].append(a)
    return dict(pdflat=np.stack(ys), state=(c, h), cache=cache, prev=prev)


def backward(p, fw, dout, rounded=True):
    """lstm_np.backward with the data and weight gradient of the cell matrix on rounded operands."""
    W = ln.unpack(p)
    lay, _ = ln.layout(ln.steps_of(p))
    g = {k: np.zeros(s) for k, (_, s) in lay.items()}
    C = fw["cache"]
    T = len(C["x"])
    dh_out = []
    for t in range(T):   # the heads: f32 arithmetic on the device, exact here
        a = C["acts"][t]
        gW, gb, da = dense_backward(a[4], dout[t], W[f"h{t}/W5"])
        g[f"h{t}/W5"] += gW
        g[f"h{t}/b5"] += gb
        for k in range(4, 0, -1):
            gW, gb, da = dense_backward(a[k - 1], tanh_grad(a[k], da), W[f"h{t}/W{k}"])
            g[f"h{t}/W{k}"] += gW
            g[f"h{t}/b{k}"] += gb
        dh_out.append(da)
    Wl = W["Wl"]
    WlT = _r(Wl, rounded).T
    dWl, dbl = np.zeros_like(Wl), np.zeros(Wl.shape[1])
    dxs = [None] * T
    dh_next = np.zeros_like(np.asarray(C["hprev"][-1], np.float64))
    dc_next = np.zeros_like(dh_next)
    for t in range(T - 1, -1, -1):
        s = dict(gi=C["gi"][t], gj=C["gj"][t], gf=C["gf"][t], go=C["go"][t], c=C["c"][t], cprev=C["cprev"][t])
        dz, dc_next = ln.cell_backward(s, dh_out[t] + dh_next, dc_next)
        xin = np.concatenate([C["x"][t], C["hprev"][t]], 1)
        dWl += _r(xin, rounded).T @ _r(dz, rounded)
        dbl += dz.reshape(-1, dz.shape[-1]).sum(0)   # the unrounded dz
        dxin = _r(dz, rounded) @ WlT
        dxs[t], dh_next = dxin[:, :ln.IN_X], dxin[:, ln.IN_X:]
    g["Wl"], g["bl"] = dWl, dbl
    for t in range(T):   # the prev_pdflat projection feeds x_t[11:43]: exact on the (rounded-product) dx
        gW, gb, _ = dense_backward(fw["prev"][t], dxs[t][:, 11:ln.IN_X], W["Wp"])
        g["Wp"] += gW
        g["bp"] += gb
    return np.concatenate([g[k].ravel() for k in lay])


def step_gradient(p, ob, prev, t, loss, state0=None, n_global=None, keep_prob=1.0, seed=0, step=0, row_base=0,
                  rounded=True):
    """One rollout: (gradient, loss, sum sq mean error, forward) of windows ob, prev, t [T,B,.] with
    input dropout keyed as the device's."""
    T, B, _ = np.asarray(ob).shape
    fw = forward(p, ln.dropout(ob, keep_prob, seed, step, row_base), prev, state0, rounded)
    lval, d, sq = ln.loss_and_dout(fw["pdflat"], t, loss, T * (n_global or B))
    return backward(p, fw, d, rounded), lval, sq, fw


def batch(T, B, seed=0):
    """tests/test_student_lstm_gpu.py's _batch."""
    rs = np.random.RandomState(seed)
    ob = rs.uniform(-1, 1, (T, B, 11)).astype(np.float32)
    prev = np.concatenate([rs.uniform(-.5, .5, (T, B, 2)), rs.uniform(-1, 0, (T, B, 2))], 2).astype(np.float32)
    t = np.concatenate([rs.uniform(-.5, .5, (T, B, 2)), rs.uniform(-1.0, -0.2, (T, B, 2))], 2).astype(np.float32)
    return ob, prev, t


def params(seed=6, T=10):
    """tests/test_student_lstm_gpu.py's _params: Glorot kernels, biases U(+-0.1)."""
    p = ln.init(seed, T)
    rs = np.random.RandomState(seed + 1)
    for k, (o, s) in ln.layout(T)[0].items():
        if len(s) == 1:
            p[o:o + s[0]] = rs.uniform(-.1, .1, s[0]).astype(np.float32)
    return p


def state(B, seed=5):
    return np.random.RandomState(seed).uniform(-.5, .5, (2, B, 200)).astype(np.float32)


def outside(got, ref):
    """Share of the outputs outside the f32 forward test's tolerance 5e-5 + 1e-4 |ref|."""
    return float(np.mean(np.abs(got - ref) > 5e-5 + 1e-4 * np.abs(ref)))


def rel_l2(g, want):
    return float(np.linalg.norm(np.asarray(g, np.float64) - want) / np.linalg.norm(want))
