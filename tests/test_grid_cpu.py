"""The inputs of the regret-grid tests (tests/test_gpu_grid.py) do what those tests need: on
the `beam` family (tests/_etas_cases.py) any two step sizes of ETAS have different sub-gradient
sign sequences — hence different θ — within the first t steps, in nearly every sequence, at
every checkpoint t >= 63.  A grid kernel that shared θ across its columns, or emitted one
column's state for another, therefore cannot pass at any checkpoint from 63 up.  NumPy only."""
import itertools

import numpy as np
import pytest

from tests import _etas_cases as E

# tests/test_gpu_grid.py's checkpoints: the ring depth, the 64-step boundaries of the U refresh
# and of the scale table, the last step and both ends
CHECKPOINTS = [0, 1, 2, 63, 64, 65, 128, 129, 256, 257]


@pytest.mark.parametrize("d", E.DIMS)
def test_beam_separates_the_step_sizes_within_every_prefix(d):
    f = E.beam(d)
    assert f.z.shape == (E.B, E.T, d) and CHECKPOINTS[-1] == E.T
    tr = {eta: E.sign_trace(f.z, f.y, eta)[0] for eta in E.ETAS}
    for a, b in itertools.combinations(E.ETAS, 2):
        ne = tr[a] != tr[b]
        for t in CHECKPOINTS:
            if t < 63:
                continue
            differ = np.any(ne[:, :t], axis=1)
            assert differ.sum() >= 20, (d, a, b, t, int(differ.sum()))
