"""The device replay ring (include/reacher_replay.h, reacherdistilation_amd/replay.py) against its NumPy
model (tests/replay_model.py): the three pushes with wrap-around, the Philox draw, the window and row
gathers, the device counters under graph replay, and the opt-in replay mode of the two train_envs
drivers.  The feature only copies floats and draws integers, so every comparison is bitwise
(np.array_equal / torch.equal); there is no tolerance anywhere."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests.replay_model import F_REW, REC, START_COMMON, START_PER_WINDOW, STEPS, RingModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RD_EINVAL = -100000
SEED = 0x0123_4567_89AB_CDEF   # both key words non-zero
CAP = 12


def _ring(capacity=CAP, max_batch=256, seed=SEED):
    from reacherdistilation_amd.replay import ReplayRing
    return ReplayRing(capacity, device=DEV, seed=seed, max_batch=max_batch), RingModel(capacity, seed)


def _teacher():
    from reacherdistilation_amd.distill import DistillConfig
    from reacherdistilation_amd.policy import synthetic_teacher
    return synthetic_teacher(DistillConfig().teacher_seed)


def _same_ring(ring, model):
    assert np.array_equal(ring.records.cpu().numpy(), model.ring)
    assert ring.counters() == (model.pushed, model.draws)
    assert ring.stored() == model.stored()


def _random_episodes(E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(E, STEPS, REC, generator=g).to(DEV)


# -- pushes ---------------------------------------------------------------------------------------
def test_push_steps_from_the_lstm_envs_wraps_like_the_model():
    from reacherdistilation_amd._native import NativeError
    from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer
    n, K = 5, 100
    st = StudentLstmTrainer(StudentLstmConfig(steps=10, max_windows=64), device=DEV)
    st.set_teacher(_teacher())
    st.attach_envs(n, seed=3, accum_steps=K)
    ring, model = _ring()
    for call in range(2):   # 10 episodes each into 12 slots: the second call wraps
        rec = st.act_envs("student", K).records.clone()
        assert tuple(rec.shape) == (K, n, REC) and bool((rec[:, :, 20] == 1).all())
        ring.push_steps(rec)
        model.push_steps(rec.cpu().numpy())
        _same_ring(ring, model)
    assert model.pushed == 20
    # episode q = (k / 50) n + i of the second call sits in slot (10 + q) % 12
    got = ring.records.cpu()
    for blk, i in itertools.product(range(2), range(n)):
        assert torch.equal(got[(10 + blk * n + i) % CAP], rec[blk * 50:(blk + 1) * 50, i].cpu())
    # (K / 50) n_envs > capacity: refused, nothing written, nothing counted
    with pytest.raises(NativeError) as e:
        ring.push_steps(torch.ones(50, 13, REC, device=DEV))
    assert f"rc={RD_EINVAL}" in str(e.value) and "rd_replay_push_steps" in str(e.value) and "capacity" in str(e.value)
    _same_ring(ring, model)
    st.close()
    ring.close()


@pytest.fixture(scope="module")
def mlp_student():
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    sm = StudentMlpTrainer(StudentMlpConfig(), device=DEV)
    sm.set_teacher(_teacher())
    yield sm
    sm.close()


def test_push_episodes_from_the_mlp_evaluation(mlp_student):
    res = mlp_student.evaluate(3, 2, seed=5, records=True)
    assert tuple(res.records.shape) == (2, 3, STEPS, REC)
    ring, model = _ring(capacity=4)
    for _ in range(2):   # 6 episodes into 4 slots, twice
        with pytest.raises(Exception):
            ring.push_episodes(res.records)          # E = 6 > capacity
        ring.push_episodes(res.records[0])
        ring.push_episodes(res.records[1])
        model.push_episodes(res.records[0].cpu().numpy())
        model.push_episodes(res.records[1].cpu().numpy())
        _same_ring(ring, model)
    assert model.pushed == 12
    ring.close()
    # the whole [E, n, 50, 21] block in one call, flattened episode-major
    ring, model = _ring(capacity=7)
    ring.push_episodes(res.records)
    model.push_episodes(res.records.cpu().numpy())
    _same_ring(ring, model)
    assert torch.equal(ring.records[:6].cpu(), res.records.reshape(6, STEPS, REC).cpu())
    ring.close()


def test_push_rows_keeps_the_rows_the_mlp_envs_emitted(mlp_student):
    sm, n, K = mlp_student, 5, 50
    sm.attach_envs(n, seed=2, accum_steps=K)
    ring, model = _ring()
    calls, carry = [], np.zeros(n, np.float32)
    for _ in range(2):
        r = sm.act_envs("student")
        c = {k: getattr(r, k).clone().cpu().numpy() for k in ("x", "t_pdflat", "s_pdflat", "reward")}
        ring.push_rows(r)                               # the carry is the ring's business
        model.push_rows(c["x"], c["t_pdflat"], c["s_pdflat"], c["reward"], carry, 1.0)
        c["carry"], carry = carry, c["reward"][-1].copy()
        calls.append(c)
    _same_ring(ring, model)
    got = ring.records.cpu().numpy()
    # sample_rows' definition applied to the ring: x = ob_s | t_{s-1} | rew_{s-1}, zeros at s = 0
    m = RingModel(CAP)
    m.ring = got
    x_all = np.concatenate([got[..., :11], m._prev()], -1)       # [capacity, 50, 16]
    for call, c in enumerate(calls):
        assert np.abs(c["carry"]).min() > 0 or call == 0
        for i in range(n):
            slot = call * n + i
            assert np.array_equal(x_all[slot], c["x"][:, i])               # every stored (episode, s)
            assert np.array_equal(got[slot, :, 12:16], c["t_pdflat"][:, i])
            assert np.array_equal(got[slot, :, 16:20], c["s_pdflat"][:, i])
            assert np.array_equal(got[slot, 1:, F_REW], c["reward"][:-1, i])   # the shifted reward
            assert got[slot, 0, F_REW] == c["carry"][i]
    # and the launch itself: drawn rows are rows some env emitted, and equal the model's
    for B, recent, base in ((67, 0, 0), (200, 3, 2 ** 33 + 5)):
        x, t, idx = (v.cpu().numpy() for v in ring.sample_rows(B, recent=recent, window_base=base, with_idx=True))
        mx, mt, midx = model.sample_rows(B, recent=recent, window_base=base)
        assert np.array_equal(idx, midx) and np.array_equal(x, mx) and np.array_equal(t, mt)
        assert np.array_equal(x, x_all[idx[:, 0], idx[:, 1]])
    # reset_carry: the next push starts from a zero carried reward again
    ring.reset_carry()
    ring.push_rows(sm.act_envs("student"))
    assert bool((ring.records[(10 + torch.arange(n)) % CAP, 0, F_REW] == 0).all())
    ring.close()


# -- draws and gathers ----------------------------------------------------------------------------
def _native_sample(ring, T, B, mode, recent, base, prew, idx):
    """rd_replay_sample_windows with caller buffers (prew / idx None: NULL pointers)."""
    from reacherdistilation_amd import _native as nat
    from reacherdistilation_amd.replay import RdReplaySample
    s = RdReplaySample(steps=T, start_mode=mode, windows=B, window_base=base, recent=recent, seed=ring.seed % 2 ** 64)
    kw = dict(dtype=torch.float32, device=DEV)
    ob, pv, tw = torch.full((T, B, 11), -7.0, **kw), torch.full((T, B, 4), -7.0, **kw), torch.full((T, B, 4), -7.0, **kw)
    ring._sync_stream()
    rc = ring._lib.rd_replay_sample_windows(ring._h, ctypes.byref(s), nat.ptr(ob), nat.ptr(pv), nat.ptr(tw),
                                            nat.ptr(prew) if prew is not None else None,
                                            nat.ptr(idx) if idx is not None else None)
    return rc, ob, pv, tw


@pytest.mark.parametrize("T", [1, 10, 50])
@pytest.mark.parametrize("fill", ["part", "wrapped"])
def test_sample_windows_equals_the_model(fill, T):
    ring, model = _ring()
    pushes = [7] if fill == "part" else [7, 9]     # 7 of 12 slots, or 16 episodes through 12 slots
    for k, E in enumerate(pushes):
        eps = _random_episodes(E, 10 + k)
        ring.push_episodes(eps)
        model.push_episodes(eps.cpu().numpy())
    _same_ring(ring, model)
    zero_prev_seen = False
    for B, mode, recent, base in itertools.product((1, 67, 200), (START_PER_WINDOW, START_COMMON), (0, 3),
                                                   (0, 2 ** 33 + 5)):
        out = ring.sample_windows(T, B, common_start=mode == START_COMMON, recent=recent, window_base=base,
                                  with_idx=True)
        want = model.sample_windows(T, B, mode, recent, base)
        for name, g, w in zip(("ob_w", "prev_w", "t_w", "prew_w", "idx"), out, want):
            assert g.cpu().numpy().dtype == w.dtype and np.array_equal(g.cpu().numpy(), w), (name, B, mode, recent, base)
        idx = want[4]
        count = min(model.stored(), recent) if recent else model.stored()
        assert set(idx[:, 0].tolist()) <= {g % CAP for g in range(model.pushed - count, model.pushed)}
        assert idx[:, 1].max() <= 50 - T
        first = idx[:, 1] == 0                       # windows from record 0: zero prev rows at position 0
        zero_prev_seen |= bool(first.any())
        assert not out[1].cpu().numpy()[0, first].any() and not out[3].cpu().numpy()[0, first].any()
        if mode == START_COMMON:
            assert len(set(idx[:, 1].tolist())) == 1
    assert zero_prev_seen
    # prew_w and idx NULL: the other outputs are what they are with them
    rc, ob, pv, tw = _native_sample(ring, T, 67, START_PER_WINDOW, 0, 5, None, None)
    assert rc == 0
    want = model.sample_windows(T, 67, START_PER_WINDOW, 0, 5)
    assert np.array_equal(ob.cpu().numpy(), want[0]) and np.array_equal(pv.cpu().numpy(), want[1])
    assert np.array_equal(tw.cpu().numpy(), want[2])
    _same_ring(ring, model)
    ring.close()


def test_sample_checks_that_read_the_handle():
    from reacherdistilation_amd._native import NativeError
    ring, model = _ring(max_batch=64)
    with pytest.raises(NativeError) as e:           # nothing was ever pushed
        ring.sample_windows(10, 8)
    assert f"rc={RD_EINVAL}" in str(e.value) and "never been pushed" in str(e.value)
    with pytest.raises(NativeError) as e:
        ring.sample_rows(8)
    assert f"rc={RD_EINVAL}" in str(e.value) and "never been pushed" in str(e.value)
    ring.push_episodes(_random_episodes(2, 1))
    with pytest.raises(ValueError):
        ring.sample_windows(10, 65)
    rc, *_ = _native_sample(ring, 10, 65, START_PER_WINDOW, 0, 0, None, None)   # B > max_batch, natively
    assert rc == RD_EINVAL and "max_batch" in ring._lib.rd_last_error().decode()
    assert ring.counters() == (2, 0)                # a refused sample draws nothing
    ring.reset()                                    # counters to 0, the floats stay
    assert ring.counters() == (0, 0) and bool(ring.records[:2].abs().sum() > 0)
    with pytest.raises(NativeError):
        ring.sample_windows(10, 8)
    ring.close()


# -- the counters live on the device --------------------------------------------------------------
def _numpy(out):
    return [v.cpu().numpy() for v in out]


def test_consecutive_samples_and_graph_replays_advance_the_draw_index():
    ring, model = _ring()
    eps = _random_episodes(7, 21)
    ring.push_episodes(eps)
    model.push_episodes(eps.cpu().numpy())
    T, B = 10, 67
    for d in range(2):                              # two consecutive samples use d and d + 1
        assert model.draws == d
        got, want = _numpy(ring.sample_windows(T, B, with_idx=True)), model.sample_windows(T, B)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert not np.array_equal(got[4], model.sample_windows(T, B)[4])   # the model's NEXT draw differs ...
    model.draws -= 1                                                   # ... (undo the look-ahead)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ring.sample_windows(T, B, with_idx=True)
    assert ring.counters() == (7, 2)                # capturing runs nothing
    for _ in range(2):                              # each replay is the NEXT draw
        g.replay()
        torch.cuda.synchronize()
        want = model.sample_windows(T, B)
        assert all(np.array_equal(a, b) for a, b in zip(_numpy(out), want))
    assert ring.counters() == (7, 4) == (model.pushed, model.draws)
    # a push captured with the sample lands in the next slots, and the draw sees the new count
    static = torch.zeros(3, STEPS, REC, device=DEV)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        ring.push_episodes(static)
        out2 = ring.sample_windows(T, B, with_idx=True)
    for k in range(2):                              # 7 + 3 + 3 episodes through 12 slots: the second wraps
        new = _random_episodes(3, 30 + k)
        static.copy_(new)
        g2.replay()
        torch.cuda.synchronize()
        model.push_episodes(new.cpu().numpy())
        want = model.sample_windows(T, B)
        assert all(np.array_equal(a, b) for a, b in zip(_numpy(out2), want))
        _same_ring(ring, model)
    assert ring.counters() == (13, 6)
    ring.close()


def _hip():
    """The HIP runtime this process already loaded (torch's), with the five graph calls' signatures."""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    hip = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    for name, args in (("hipStreamBeginCapture", [vp, ctypes.c_int]), ("hipStreamEndCapture", [vp, ctypes.POINTER(vp)]),
                       ("hipGraphGetNodes", [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]),
                       ("hipGraphGetEdges", [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz)]),
                       ("hipGraphNodeGetType", [vp, ctypes.POINTER(ctypes.c_int)]), ("hipGraphDestroy", [vp])):
        getattr(hip, name).argtypes, getattr(hip, name).restype = args, ctypes.c_int
    return hip


def test_a_captured_sample_is_a_single_chain():
    """The draw, gather and bump launches of one sample go to one stream: captured, they are three
    kernel nodes in one chain, no parallel branches (read from the captured hipGraph itself)."""
    hip = _hip()
    ring, _ = _ring()
    ring.push_episodes(_random_episodes(7, 40))
    ring.sample_windows(10, 67)                     # the output buffers exist before the capture
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(DEV)
    graph = ctypes.c_void_p()
    with torch.cuda.stream(stream):
        assert hip.hipStreamBeginCapture(stream.cuda_stream, 2) == 0      # hipStreamCaptureModeRelaxed
        try:
            ring.sample_windows(10, 67)
        finally:
            rc = hip.hipStreamEndCapture(stream.cuda_stream, ctypes.byref(graph))
    assert rc == 0 and graph.value
    assert ring.counters() == (7, 1)                # capturing ran nothing
    n = ctypes.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0 and n.value == 3
    nodes = (ctypes.c_void_p * 3)()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
    kind = ctypes.c_int(-1)
    for node in nodes:
        assert hip.hipGraphNodeGetType(node, ctypes.byref(kind)) == 0 and kind.value == 0   # hipGraphNodeTypeKernel
    e = ctypes.c_size_t()
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(e)) == 0 and e.value == 2
    src, dst = (ctypes.c_void_p * 2)(), (ctypes.c_void_p * 2)()
    assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(e)) == 0
    src, dst = list(src), list(dst)
    assert len(set(src)) == 2 and len(set(dst)) == 2            # nobody has two successors or two predecessors
    assert len(set(src) | set(dst)) == 3 and len(set(src) & set(dst)) == 1   # a -> b -> c
    assert hip.hipGraphDestroy(graph) == 0
    ring.close()


# -- the drivers ----------------------------------------------------------------------------------
def _lstm_trainer(max_windows, steps, dtype):
    from reacherdistilation_amd.student_lstm import StudentLstmConfig, StudentLstmTrainer
    st = StudentLstmTrainer(StudentLstmConfig(loss="kl", lr=1e-3, keep_prob=1.0, seed=0, steps=10,
                                              max_windows=max_windows, metrics_len=steps, dtype=dtype), device=DEV)
    st.set_teacher(_teacher())
    st.attach_envs(4, seed=0, accum_steps=50)
    return st


def _mlp_trainer(steps, dtype):
    from reacherdistilation_amd.student_mlp import StudentMlpConfig, StudentMlpTrainer
    sm = StudentMlpTrainer(StudentMlpConfig(loss="kl", lr=1e-4, keep_prob=1.0, seed=0, metrics_len=steps, dtype=dtype),
                           device=DEV)
    sm.set_teacher(_teacher())
    sm.attach_envs(4, seed=0, accum_steps=50)
    return sm


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lstm_train_envs_with_a_ring_is_the_hand_written_loop(dtype):
    from reacherdistilation_amd import lstm_train
    from reacherdistilation_amd.replay import ReplayRing
    st, hist = lstm_train.train_envs(4, 2, replay_capacity=8, replay_windows=24, updates_per_act=2, dtype=dtype,
                                     device=DEV)
    assert st.cfg.max_windows == 24 and len(hist) == 2 and st.counter() == 2
    assert st.replay.counters() == (4, 2)
    ref = _lstm_trainer(24, 2, dtype)
    ring = ReplayRing(8, device=DEV, seed=0, max_batch=24)
    ring.push_steps(ref.act_envs("student").records)
    for _ in range(2):
        ob_w, prev_w, t_w, _ = ring.sample_windows(10, 24)
        ref.step(ob_w, prev_w, t_w)
    assert torch.equal(st.params(), ref.params())
    assert np.array_equal(st.metrics(2), ref.metrics(2))
    assert torch.equal(st.replay.records, ring.records)
    assert not torch.equal(st.params(), _lstm_trainer(24, 2, dtype).params())   # it did train


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mlp_train_envs_with_a_ring_is_the_hand_written_loop(dtype):
    from reacherdistilation_amd import mlp_train
    from reacherdistilation_amd.replay import ReplayRing
    sm, hist = mlp_train.train_envs(4, 2, replay_capacity=8, replay_windows=24, updates_per_act=2, dtype=dtype,
                                    device=DEV)
    assert len(hist) == 2 and sm.counter() == 2 and sm.replay.counters() == (4, 2)
    ref = _mlp_trainer(2, dtype)
    ring = ReplayRing(8, device=DEV, seed=0, max_batch=24)
    ring.push_rows(ref.act_envs("student"))
    for _ in range(2):
        ref.step(*ring.sample_rows(24))
    assert torch.equal(sm.params(), ref.params())
    assert np.array_equal(sm.metrics(2), ref.metrics(2))
    assert torch.equal(sm.replay.records, ring.records)
    assert not torch.equal(sm.params(), _mlp_trainer(2, dtype).params())


def test_train_envs_without_a_ring_is_the_step_envs_loop():
    """replay_capacity = 0 (the default): what the drivers did before the ring existed."""
    from reacherdistilation_amd import lstm_train, mlp_train
    st, hist = lstm_train.train_envs(4, 2, device=DEV)
    ref = _lstm_trainer(4 * 41, 2, "f32")
    rew = [float(ref.step_envs("student").reward.mean()) for _ in range(2)]
    assert torch.equal(st.params(), ref.params()) and np.array_equal(st.metrics(2), ref.metrics(2))
    assert [h[3] for h in hist] == rew and not hasattr(st, "replay")
    sm, hist = mlp_train.train_envs(4, 2, device=DEV)
    ref = _mlp_trainer(2, "f32")
    rew = [float(ref.step_envs("student").reward.mean()) for _ in range(2)]
    assert torch.equal(sm.params(), ref.params()) and np.array_equal(sm.metrics(2), ref.metrics(2))
    assert [h[3] for h in hist] == rew and not hasattr(sm, "replay")
