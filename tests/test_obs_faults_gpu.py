"""rd_mask_obs (include/reacher_obs_faults.h; obs_faults.mask_obs), the stepwise primitive of the sensor
faults, against the NumPy model of tests/obs_faults.py: seen and kept are the model's bit for bit
(np.array_equal) -- the mask is integer arithmetic and one comparison, a kept reading is itself or one
correctly rounded f32 division, so there is no tolerance to state."""
import numpy as np
import pytest
import torch

from tests import obs_faults as of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n", [1, 17, 83])
def test_mask_obs_equals_the_numpy_model(n):
    """Env ids that cross 2^32 and a seed with a high word, at episode 3 step 49 and episode 0 step 0, in
    the three modes, at keep_prob 0.5 (the suites'), 0.9 (a quotient that rounds) and 1."""
    from reacherdistilation_amd.obs_faults import mask_obs
    rs = np.random.RandomState(n)
    ob = rs.uniform(-2.0, 2.0, (n, of.OB)).astype(np.float32)
    ob[:, 10] = 0.0   # as the env's
    base = of.WIDE_BASE + 40 - n // 2   # the ids straddle 2^32 (for n = 1: 2^32 itself)
    assert base <= 2 ** 32 <= base + n
    dev = torch.from_numpy(ob).to(DEV)
    for episode, step in ((3, 49), (0, 0)):
        for keep_prob in (0.5, 0.9, 1.0):
            keep = of.kept(of.WIDE_SEED, base, n, episode, step, keep_prob)
            for mode in ("dropout", "missing", "none"):
                seen, kept = mask_obs(dev, mode=mode, keep_prob=keep_prob, seed=of.WIDE_SEED, env_base=base,
                                      episode=episode, step=step, return_kept=True)
                assert kept.dtype == torch.uint8 and seen.shape == kept.shape == (n, of.OB)
                assert np.array_equal(kept.cpu().numpy().astype(bool), keep), (episode, keep_prob, mode)
                want = of.see(ob, keep, of.MODES[mode], keep_prob)
                assert np.array_equal(seen.cpu().numpy().view(np.uint32), want.view(np.uint32)), (episode, keep_prob, mode)
                if keep_prob == 1.0 or mode == "none":
                    assert torch.equal(seen, dev)
    assert torch.equal(mask_obs(dev, mode="missing", keep_prob=0.5, seed=of.WIDE_SEED, env_base=base, step=7),
                       mask_obs(dev, mode="missing", keep_prob=0.5, seed=of.WIDE_SEED, env_base=base, step=7))


def test_mask_obs_is_a_function_of_the_env_id_not_of_the_launch():
    """the rows of a 83-env call equal those of calls on its parts (one block of 256 threads and its tail)"""
    from reacherdistilation_amd.obs_faults import mask_obs
    rs = np.random.RandomState(5)
    ob = torch.from_numpy(rs.uniform(-2.0, 2.0, (300, of.OB)).astype(np.float32)).to(DEV)
    kw = dict(mode="dropout", keep_prob=0.5, seed=11, episode=1, step=13)
    whole = mask_obs(ob, env_base=5, **kw)
    assert torch.equal(whole[:17], mask_obs(ob[:17], env_base=5, **kw))
    assert torch.equal(whole[250:], mask_obs(ob[250:], env_base=255, **kw))
    assert 0.4 < float((whole != 0).float()[:, :10].mean()) < 0.6
