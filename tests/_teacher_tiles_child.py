"""Child process of tests/test_teacher_tiles_gpu.py: tests/_det_child.py's harness (two fresh trainers
per case, two fused steps each, sha256 of gradient, parameters and env state) on the teacher_tiles
masks at 4,160 envs in 64-env groups on 8 workgroups: pair 0 owns three groups, the others two."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _det_child  # noqa: E402

CASES = {f"tt{m}_n4160": dict(n_envs=4160, grid=8, group_envs=64, f32_split=True, teacher_tiles=m)
         for m in (0b0010, 0b1010, 0b1110)}

if __name__ == "__main__":
    _det_child.CASES.update(CASES)
    _det_child.main(list(CASES))
