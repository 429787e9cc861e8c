"""CPU mutation test of the two reference students' gradient check (tests/student_parity.py): at
every (loss, shape) at which the GPU tests compare a gradient the per-entry bound passes a
correct f32 result and rejects each way a weight-gradient sum can lose a part, and the bounds the
four GPU files had alone (kept here as _old_mlp_check / _old_lstm_check) accept them at the
largest shapes.

The "kernel result" is the oracle's own gradient (in the bf16 modes the emulation's) carried
through f32.  Mutations, each built from student_parity.row_contribution on the forward computed
once per case:
  * one row (MLP) or one window (LSTM) lost, at indices 15, 63 and n - 1;
  * batch rows 12-15 of the last whole 16-row tile lost in one layer's dW: each of the five MLP
    layers, head 0's dW5 for the LSTM (the lanes 48-63 of a wave in a 16-row tile);
  * one row lost in layer 0's dW only, and in layer 1's;
  * one window's t = 0 term of dWl and its t = 1 term of dWp (t = 0 where T = 1);
  * the last K mod 16 rows of the K = T B rows of dWl's sum, all at t = T - 1 (where K is a
    multiple of 16: the last 4, one k step of the MFMA);
  * head 2's dW3 losing one window (the last head where T < 3).
Every case is judged with the verdict in force for its shape (student_parity.in_force), so raising
a tolerance past a mutation fails here, and the caps of student_parity.py are held to half of the
weakest mutation at the largest shapes.  Where the bf16 bounds are not in force (under 2,000 rows
the device's rounding flips alone exceed the cap) every mutation is shown to measure more than the
cap.  The old bounds at the largest shapes, with the GPU tests' own batches: the MLP's accept one
row lost in layer 0's or layer 1's dW under either loss, and under kl a whole lost row and the
four tile rows of any layer (under mse its max-abs bound sees those two); the LSTM's accept every
partial mutation under either loss and reject most whole windows.
"""
import functools

import numpy as np
import pytest

from oracle import lstm_np as ln
from oracle import refnet_np as rn
from tests import lstm_bf16 as lb
from tests import refnet_bf16 as rb
from tests import student_parity as sp

# the shapes at which tests/test_student_{mlp,lstm}{,_bf16}_gpu.py compare a gradient
MLP_NS = {"f32": [1, 15, 16, 17, 20, 63, 64, 65, 129, 200, 500, 1000, 20000],
          "bf16": [1, 15, 16, 17, 20, 63, 64, 65, 129, 200, 330, 1000]}
LSTM_SHAPES = {"f32": [(10, 16), (10, 20), (10, 31), (10, 32), (10, 33), (2, 17), (10, 53), (10, 50), (10, 60), (5, 40),
                       (1, 7), (3, 1), (16, 24), (40, 17), (10, 300), (4, 2000)],
               "bf16": [(10, 1), (10, 20), (10, 31), (10, 33), (10, 53), (10, 65), (10, 50), (10, 60), (5, 40), (1, 7), (4, 330),
                        (4, 2000)]}
MLP_LARGEST, LSTM_LARGEST = 20000, (4, 2000)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _old_mlp_check(g, want):
    """tests/test_student_mlp{,_bf16}_gpu.py's _grad_check before the per-entry bound."""
    rel = np.linalg.norm(g - want) / np.linalg.norm(want)
    return rel < 2e-4 and np.abs(g - want).max() <= 1e-4 * np.abs(want).max() + 1e-6


def _old_lstm_check(g, want):
    """tests/test_student_lstm{,_bf16}_gpu.py's."""
    rel = np.linalg.norm(g - want) / np.linalg.norm(want)
    return rel < 5e-4 and np.abs(g - want).max() <= 1e-3 * np.abs(want).max() + 1e-6


@functools.lru_cache(maxsize=None)
def _mlp_case(mode, loss, n):
    if mode == "f32":
        from tests.test_student_mlp_gpu import _batch, _params
        x, t = _batch(n, 7 + n)
        return sp.mlp_reference(_params(), x, t, loss)
    x, t = rb.batch(n, 7 + n)
    return sp.mlp_reference(rb.params(), x, t, loss, rounded=rb.BF_LAYERS)


@functools.lru_cache(maxsize=None)
def _lstm_case(mode, loss, T, B):
    ob, prev, t = lb.batch(T, B, 3 + B)
    return sp.lstm_reference(lb.params(T=T), ob, prev, t, loss, rounded=mode == "bf16")


def _tile_rows(n):
    """Batch rows 12-15 of the last whole 16-row tile ([] under 16 rows)."""
    t0 = (n // 16 - 1) * 16
    return list(range(t0 + 12, t0 + 16)) if n >= 16 else []


def mlp_mutations(ref, n):
    """{name: the part of the gradient that is lost}."""
    pr = ref["products"]
    c = functools.partial(sp.row_contribution, pr, rn.P_REF)
    out = {f"row {r} lost": c([r]) for r in sorted({r for r in (15, 63, n - 1) if r < n})}
    r = min(63, n - 1)
    out["one row of layer 0's dW"] = c([r], only="W0")
    out["one row of layer 1's dW"] = c([r], only="W1")
    if _tile_rows(n):
        for li in range(5):
            out[f"tile rows 12-15 of layer {li}'s dW"] = c(_tile_rows(n), only=f"W{li}")
    return out


def lstm_mutations(ref, T, B):
    pr = ref["products"]
    c = functools.partial(sp.row_contribution, pr, ref["size"])
    out = {f"window {w} lost": c([w]) for w in sorted({w for w in (15, 63, B - 1) if w < B})}
    w = min(63, B - 1)
    out["one window's t=0 term of dWl"] = c([w], only=("Wl", 0))
    out["one window's t=1 term of dWp"] = c([w], only=("Wp", min(1, T - 1)))
    tail = (T * B) % 16 or 4
    out["the last K mod 16 rows of dWl"] = c(list(range(max(0, B - tail), B)), only=("Wl", T - 1))
    out["one window of head 2's dW3"] = c([w], only=(f"h{min(2, T - 1)}/W3", None))
    if _tile_rows(B):
        out["tile rows 12-15 of head 0's dW5"] = c(_tile_rows(B), only=("h0/W5", None))
    return out


def _judge(ref, muts, bf16, label, rows):
    """The stand-in passes; every mutation is rejected by the verdict in force for `rows` rows per
    product.  Where the bf16 bounds are not in force (student_parity.in_force: under BF16_MIN_ROWS
    rows the device's rounding flips alone exceed the cap), every mutation still measures more
    than the cap.  Returns {name: per-entry error}."""
    g64, M = ref["g64"], ref["M"]
    ok, rep = sp.grad_ok(_f32(g64), g64, M, rows, bf16)
    assert ok and rep["entry"] <= 6e-8 and rep["global"] <= 6e-8, (label, rep)
    cap = sp.tolerances(g64.size, bf16)[2]
    worst = {}
    for what, lost in muts.items():
        ok, rep = sp.grad_ok(_f32(g64 - lost), g64, M, rows, bf16)
        if bf16 and not sp.in_force(rows, bf16)[0]:
            assert rep["entry"] > cap, (label, what, rep)
        else:
            assert not ok, (label, what, rep)
        worst[what] = rep["entry"]
    print(label, {k: f"{v:.1e}" for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_mlp_clean_gradient_passes_and_each_mutation_is_rejected(mode, loss):
    for n in MLP_NS[mode]:
        ref = _mlp_case(mode, loss, n)
        assert int((ref["M"] == 0).sum()) == (66 if loss == "mse" else 0)
        _judge(ref, mlp_mutations(ref, n), mode == "bf16", f"mlp {mode} {loss} n={n}", n)


@pytest.mark.parametrize("loss", ["mse", "kl"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_lstm_clean_gradient_passes_and_each_mutation_is_rejected(mode, loss):
    for T, B in LSTM_SHAPES[mode]:
        ref = _lstm_case(mode, loss, T, B)
        # one step from a zero state: h_0 = c_0 = 0, so Wl's 200 recurrent rows and the forget gate's
        # columns (dz_f = dc c_0 ..) have no contribution at all
        start = 200 * 800 + 43 * 200 + 200 if T == 1 else 0
        assert int((ref["M"] == 0).sum()) == (66 * T if loss == "mse" else 0) + start
        _judge(ref, lstm_mutations(ref, T, B), mode == "bf16", f"lstm {mode} {loss} ({T},{B})", B)


def test_products_sum_to_the_oracles_and_the_emulations_gradients():
    """The mutations and M are built from student_parity's products: over all rows they are
    refnet_np.backward / lstm_np.backward themselves, and with `rounded` the emulations'."""
    for loss in ("mse", "kl"):
        x, t = rb.batch(203, 1)
        p = rb.params()
        for rounded in ((), rb.BF_LAYERS):
            want, _, _ = rb.step_gradient(p, x, t, loss, rounded=rounded)
            ref = sp.mlp_reference(p, x, t, loss, rounded=rounded)
            assert np.abs(ref["g64"] - want).max() <= 1e-13 * np.abs(want).max()
            every = sp.row_contribution(ref["products"], rn.P_REF, np.arange(203))
            assert np.array_equal(every, ref["g64"])
        want = rn.backward(p, rn.forward(p, x), rn.loss_and_dout(rn.forward(p, x)["pdflat"], t, loss, 203)[1])
        assert np.abs(sp.mlp_reference(p, x, t, loss)["g64"] - want).max() <= 1e-13 * np.abs(want).max()
        ob, prev, tt = lb.batch(3, 37, 2)
        pl, st = lb.params(T=3), lb.state(37)
        for rounded in (False, True):
            want, _, _, _ = lb.step_gradient(pl, ob, prev, tt, loss, st, rounded=rounded)
            ref = sp.lstm_reference(pl, ob, prev, tt, loss, st, rounded=rounded)
            assert np.abs(ref["g64"] - want).max() <= 1e-13 * np.abs(want).max()
        fw = ln.forward(pl, ob, prev, st)
        want = ln.backward(pl, fw, ln.loss_and_dout(fw["pdflat"], tt, loss, 3 * 37)[1])
        assert np.abs(sp.lstm_reference(pl, ob, prev, tt, loss, st)["g64"] - want).max() <= 1e-13 * np.abs(want).max()


def test_block_names_and_report():
    lay, n = sp.mlp_layout()
    assert n == rn.P_REF and list(lay)[:4] == ["W0", "b0", "W1", "b1"] and lay["W4"][1] == (32, 4)
    assert list(sp.lstm_layout(2)[0]) == ["Wp", "bp", "Wl", "bl"] + [f"h{t}/{w}{k}" for t in range(2)
                                                                    for k in range(1, 6) for w in "Wb"]
    ref = _mlp_case("f32", "mse", 64)
    g = ref["g64"].copy()
    k = lay["W2"][0] + 5 * 128 + 7
    g[k] += 1e-3 * ref["M"][k]
    rep = sp.grad_report(g, ref["g64"], ref["M"])
    assert (rep["block"], rep["index"], rep["worst_entry"]) == ("W2", (5, 7), k) and rep["entry"] == pytest.approx(1e-3)
    g = ref["g64"].copy()
    zero = int(np.flatnonzero(ref["M"] == 0)[0])
    g[zero] = 1e-30                                       # where M_e = 0 the entry is exactly 0
    rep = sp.grad_report(g, ref["g64"], ref["M"])
    assert rep["entry"] == np.inf and rep["block"] == "W4"
    for rows, bf16 in ((64, False), (1, False), (64, True), (4000, True)):     # asserted whatever else is in force
        assert not sp.grad_ok(g, ref["g64"], ref["M"], rows, bf16)[0]
        assert sp.grad_ok(ref["g64"], ref["g64"], ref["M"], rows, bf16)[0]


def test_the_old_bounds_accept_the_recorded_mutations_and_the_caps_are_half_the_weakest():
    """At MLP 20,000 rows and LSTM (4, 2000), the largest gradient cases of the GPU tests: the
    bounds the GPU files had accept what the per-entry bound rejects, and each TOL_CAP is half
    of the weakest mutation's per-entry error there (to the two figures it is written with)."""
    n = MLP_LARGEST
    weakest = np.inf
    for loss in ("mse", "kl"):
        ref = _mlp_case("f32", loss, n)
        muts = mlp_mutations(ref, n)
        worst = _judge(ref, muts, False, f"mlp f32 {loss} n={n}", n)
        weakest = min(weakest, *worst.values())
        old = {k: _old_mlp_check(_f32(ref["g64"] - v), ref["g64"]) for k, v in muts.items()}
        print("old MLP check accepts:", loss, [k for k, v in old.items() if v])
        assert old["one row of layer 0's dW"] and old["one row of layer 1's dW"], old
        if loss == "kl":     # under mse the old max-abs bound sees a whole row and the four tile rows of this batch
            assert all(old[f"row {r} lost"] for r in (15, 63, n - 1)), old
            assert all(old[f"tile rows 12-15 of layer {li}'s dW"] for li in range(5)), old
    print(f"MLP n={n}: weakest mutation {weakest:.3e}, cap {sp.TOL_CAP_MLP:.1e}")
    assert 0.9 * weakest / 2 <= sp.TOL_CAP_MLP <= weakest / 2, weakest
    T, B = LSTM_LARGEST
    weakest = np.inf
    for loss in ("mse", "kl"):
        ref = _lstm_case("f32", loss, T, B)
        muts = lstm_mutations(ref, T, B)
        worst = _judge(ref, muts, False, f"lstm f32 {loss} ({T},{B})", B)
        weakest = min(weakest, *worst.values())
        old = {k: _old_lstm_check(_f32(ref["g64"] - v), ref["g64"]) for k, v in muts.items()}
        print("old LSTM check accepts:", loss, [k for k, v in old.items() if v])
        for what in ("one window's t=0 term of dWl", "one window's t=1 term of dWp", "one window of head 2's dW3",
                     "the last K mod 16 rows of dWl", "tile rows 12-15 of head 0's dW5"):
            assert old[what], (loss, what, old)
    print(f"LSTM ({T},{B}): weakest mutation {weakest:.3e}, cap {sp.TOL_CAP_LSTM:.1e}")
    assert 0.9 * weakest / 2 <= sp.TOL_CAP_LSTM <= weakest / 2, weakest
    assert max(sp.TOL_ENTRY_MLP, sp.TOL_GLOBAL, sp.TOL_GLOBAL_BF16) <= sp.TOL_CAP_MLP <= sp.TOL_CAP_LSTM
    assert max(sp.TOL_ENTRY_LSTM, sp.TOL_ENTRY_BF16) <= sp.TOL_CAP_LSTM
    for size in (rn.P_REF, ln.P_LSTM):
        for bf16 in (False, True):
            te, tg, cap = sp.tolerances(size, bf16)
            assert te <= cap and tg <= cap


# ---------------------------------------------------------------- the GPU isolation tests' bound


def _isolation(ref_all, ref_e, size, r, z_row, lanes_block, lanes_shape, label):
    """g(batch) - g(batch with r replaced by z), both through f32, against the oracle's
    c(x_r) - c(z): inside the bound; with r's lanes-48-63 share of one dW removed, outside."""
    pa, pe = ref_all["products"], ref_e["products"]
    d64 = ref_all["g64"] - ref_e["g64"]
    cx, cz = sp.row_contribution(pa, size, [r]), sp.row_contribution(pe, size, [z_row])
    assert np.abs(d64 - (cx - cz)).max() <= 1e-12 * np.abs(d64).max()       # what the GPU test compares with
    bound = sp.isolation_bound(sp.scale(pa, size, [r]), sp.scale(pe, size, [z_row]), ref_all["M"], ref_e["M"])
    d32 = _f32(ref_all["g64"]) - _f32(ref_e["g64"])
    ratio, _ = sp.isolation_ratio(d32, d64, bound)
    assert ratio <= 0.25, (label, r, ratio)
    lay = sp._layout_of(size)[0]
    lost = np.zeros(size)
    sl = sp.block_slice(lay, lanes_block if isinstance(lanes_block, str) else lanes_block[0])
    share = sp.row_contribution(pa, size, [r], only=lanes_block)[sl].reshape(lanes_shape)
    lanes = np.arange(lanes_shape[0]) % 16 >= 12          # the rows of a dW that lanes 48-63 of a 16-row MFMA tile own
    lost[sl] = np.where(lanes[:, None], share, 0.0).ravel()
    ratio, k = sp.isolation_ratio(d32 - lost, d64, bound)
    assert ratio > 1.0, (label, r, ratio)
    return ratio


@pytest.mark.parametrize("loss", ["mse", "kl"])
def test_mlp_row_isolation_rejects_a_wrong_lane_group(loss):
    n = 64
    x, t = rb.batch(n, 31)
    ref = sp.mlp_reference(rb.params(), x, t, loss)
    weakest = np.inf
    for r in range(n):
        xe, te = x.copy(), t.copy()
        xe[r], te[r] = sp.ISO_MLP_Z
        ref_e = sp.mlp_reference(rb.params(), xe, te, loss)
        weakest = min(weakest, _isolation(ref, ref_e, rn.P_REF, r, r, "W2", (128, 128), f"mlp {loss}"))
    print(f"mlp {loss}: weakest lanes-48-63 mutation at {weakest:.1f} x the isolation bound")


@pytest.mark.parametrize("B", [16, 32, 33])
def test_lstm_window_isolation_rejects_a_wrong_lane_group(B):
    T = 10
    ob, prev, t = lb.batch(T, B, 41 + B)
    p = lb.params(T=T)
    ref = sp.lstm_reference(p, ob, prev, t, "kl")
    weakest = np.inf
    for r in (0, 15, B - 1):
        obe, preve, te = ob.copy(), prev.copy(), t.copy()
        obe[:, r], preve[:, r], te[:, r] = sp.iso_lstm_z(T)
        ref_e = sp.lstm_reference(p, obe, preve, te, "kl")
        weakest = min(weakest, _isolation(ref, ref_e, p.size, r, r, ("Wl", 3), (243, 800), f"lstm B={B}"))
    print(f"lstm B={B}: weakest lanes-48-63 mutation at {weakest:.1f} x the isolation bound")


def test_the_small_bf16_batches_have_no_operand_on_a_rounding_tie():
    """student_parity.mlp_bf16_seed, the batches of the bf16 block-edge cases of at most 20 rows:
    the seeds it passes over have a near-tie operand, the one it returns has none, and seed 22 at
    15 rows is the exact tie whose flip is a relative L2 of 3.1e-4 under mse."""
    p = rb.params()
    for n in (15, 16, 17):
        seed = sp.mlp_bf16_seed(n, 7 + n)
        assert sp.mlp_bf16_tie_distance(p, rb.batch(n, seed)[0]) > sp.TIE_ULPS
        assert all(sp.mlp_bf16_tie_distance(p, rb.batch(n, s)[0]) <= sp.TIE_ULPS for s in range(7 + n, seed))
        print(f"n={n}: seed {seed}")
    x, t = rb.batch(15, 22)
    assert sp.mlp_bf16_tie_distance(p, x) == 0
    fw = rb.forward(p, x)
    h = fw["hs"][2].astype(np.float32)
    assert (h.view(np.uint32)[3, 26] & 0xFFFF) == 0x8000
    g0, _, _ = rb.step_gradient(p, x, t, "mse")
    # the same step with that one operand an f32 ulp to the other side of the tie
    hs = list(fw["hs"][:3])
    hs[2] = hs[2].copy()
    rounded = rb._r(fw["hs"][2], True)[3, 26]
    hs[2][3, 26] = float(np.nextafter(h[3, 26], np.float32(-np.inf if rounded > h[3, 26] else np.inf)))
    assert rb._r(hs[2], True)[3, 26] != rounded
    for li in range(2, 5):
        (W, b), on = rn.unpack(np.asarray(p, np.float64))[li], li in rb.BF_LAYERS
        z = rb._r(hs[li], on) @ rb._r(W, on) + b
        hs.append(np.tanh(z) if rn.ACT[li] else z)
    d = rn.loss_and_dout(hs[-1], t, "mse", 15)[1]
    rel = rb.rel_l2(rb.backward(p, dict(hs=hs, pdflat=hs[-1]), d), g0)
    assert 2e-4 < rel < 4e-4, rel
