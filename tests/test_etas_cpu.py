"""The `beam` family (tests/_etas_cases.py) does what the step-size sweep tests need: on it
the step sizes of ETAS have different sub-gradient sign sequences — hence different θ
trajectories — in nearly every sequence, and both rescale regimes occur.  A kernel that shared
θ across its columns therefore cannot pass tests/test_gpu_etas.py.  NumPy only."""
import itertools

import numpy as np
import pytest

from tests import _etas_cases as E


@pytest.mark.parametrize("d", E.DIMS)
def test_beam_separates_the_step_sizes(d):
    f = E.beam(d)
    assert f.z.shape == (E.B, E.T, d) and f.y.shape == (E.B, E.T)
    assert set(np.unique(f.y)) == {-1.0, 1.0}
    nrm = np.linalg.norm(f.z, axis=2)
    assert np.all(nrm > 1.0)   # every row outside the unit ball
    tr = {eta: E.sign_trace(f.z, f.y, eta) for eta in E.ETAS}
    for a, b in itertools.combinations(E.ETAS, 2):
        differ = np.any(tr[a][0] != tr[b][0], axis=1)
        assert differ.sum() >= 20, (d, a, b, int(differ.sum()))
    # both rescale regimes: never at the smallest step size, on most steps at the largest
    assert not tr[0.25][1].any()
    assert tr[8.0][1].mean() >= 0.5


def test_usual_rows_do_not_separate_them():
    """The control: on gt_like rows every step size has the same sign sequence (-y), which is
    why the sweep tests need `beam`."""
    from tests import _families as F
    f = F.make("gt_like", E.B, E.T, 16, 116)
    for eta in E.ETAS:
        signs, _ = E.sign_trace(f.z, f.y, eta)
        assert np.array_equal(signs, -f.y)


def test_cert_case_edits_share_wave_groups_with_unedited_sequences():
    from tests import _families as F
    f, edits, two = E.cert_etas_case(64)
    for P, _ in F.CERT_SHAPES:
        S = 64 // P
        if S == 1:
            continue
        for b in two:
            mates = [m for m in range(b // S * S, b // S * S + S) if m != b and m < f.y.shape[0]]
            assert any(m not in edits and m not in two for m in mates), (P, b)
    # step 1 in the reference's order, in Python floats: the action at the two step sizes
    th = -0.5
    assert -(E.SQ2 / np.sqrt(2.0)) * th == 0.5
    x = -((4.0 * E.SQ2) / np.sqrt(2.0)) * th
    assert x == 2.0 and x * (1.0 / np.sqrt(x * x)) == 1.0
