"""The bf16 mixed-precision arithmetic of the reference MLP student (rdm_create_dtype's
RDM_DTYPE_BF16, include/reacher_student_mlp.h "Arithmetic"), restated layer-wise on the oracle's
building blocks (oracle/refnet_np.py, oracle/policy_np.bf16) with f64 sums.

Layers in ``rounded`` (default 1, 2, 3: 24->128, 128->128, 128->32) round their matrix operands to
bf16 (round-to-nearest-even): x and W in the forward, dZ and W in the data gradient, H and dZ in the
weight gradient.  Biases, tanh, the loss, db (the unrounded dZ summed) and tanh' (on the unrounded
activation) are exact.  With ``rounded=()`` this is refnet_np.forward / backward, operation for
operation.
"""
import numpy as np

from oracle import policy_np as pn
from oracle import refnet_np as rn

BF_LAYERS = (1, 2, 3)


def _r(a, on):
    return pn.bf16(a) if on else a


def forward(p, x, rounded=BF_LAYERS):
    """x [n,16] -> dict(hs=[h0..h5] (unrounded activations), pdflat [n,4])."""
    hs = [np.asarray(x, np.float64)]
    for li, ((W, b), act) in enumerate(zip(rn.unpack(np.asarray(p, np.float64)), rn.ACT)):
        on = li in rounded
        z = _r(hs[-1], on) @ _r(W, on) + b
        hs.append(np.tanh(z) if act else z)
    return dict(hs=hs, pdflat=hs[-1])


def backward(p, fw, dout, rounded=BF_LAYERS):
    Ws = rn.unpack(np.asarray(p, np.float64))
    hs = fw["hs"]
    g = [None] * len(Ws)
    dz = dout
    for li in range(len(Ws) - 1, -1, -1):
        W, _ = Ws[li]
        on = li in rounded
        gw, _, dh = rn.dense_backward(_r(hs[li], on), _r(dz, on), _r(W, on))
        _, gb, _ = rn.dense_backward(hs[li], dz, W)   # db sums the unrounded dZ
        g[li] = (gw, gb)
        if li > 0:
            dz = rn.tanh_grad(hs[li], dh) if rn.ACT[li - 1] else dh
    return np.concatenate([np.concatenate([gw.ravel(), gb]) for gw, gb in g])


def step_gradient(p, x, t, loss, n_global=None, keep_prob=1.0, seed=0, step=0, row_base=0, rounded=BF_LAYERS):
    """One training launch: (gradient, loss, sum sq mean error) on rows x with input dropout."""
    xd = rn.dropout(x, keep_prob, seed=seed, step=step, row_base=row_base)
    fw = forward(p, xd, rounded)
    lval, d, sq = rn.loss_and_dout(fw["pdflat"], t, loss, n_global or len(x))
    return backward(p, fw, d, rounded), lval, sq


def params(seed=2):
    """Glorot kernels (refnet_np.init) with biases U(+-0.2)."""
    p = rn.init(seed)
    rs = np.random.RandomState(seed + 100)
    for (_, bo, _, b) in rn.LAYOUT:
        p[bo:bo + b] = rs.uniform(-.2, .2, b).astype(np.float32)
    return p


def batch(n, seed=0):
    """Rows as the student sees them: obs U(+-1) | prev pdflat N(0, 0.5) | reward U(-0.5, 0); targets
    mean N(0, 0.5) | log-std U(-3.4, -3.2)."""
    rs = np.random.RandomState(seed)
    x = np.concatenate([rs.uniform(-1, 1, (n, 11)), rs.normal(0, .5, (n, 4)), rs.uniform(-.5, 0, (n, 1))], 1)
    t = np.concatenate([rs.normal(0, .5, (n, 2)), rs.uniform(-3.4, -3.2, (n, 2))], 1)
    return x.astype(np.float32), t.astype(np.float32)


def outside(got, ref):
    """Share of the outputs outside the f32 forward test's tolerance 2e-5 + 1e-4 |ref|."""
    return float(np.mean(np.abs(got - ref) > 2e-5 + 1e-4 * np.abs(ref)))


def rel_l2(g, want):
    return float(np.linalg.norm(np.asarray(g, np.float64) - want) / np.linalg.norm(want))
