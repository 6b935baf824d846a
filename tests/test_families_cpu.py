"""The input families of tests/_families.py reach the branches they are built for.

Every condition below is on the inputs, read from the NumPy step trace (the reference
arithmetic, fast_algorithms.py:88-115) — none is a tolerance on a kernel.  The GPU tests of
tests/test_gpu_alg_branches.py take their inputs from the same case lists, so what is shown
here for an input holds for the run that uses it:

  * the trace is the oracle's run: its regret agrees with the C oracle within 1e-12 relative;
  * no step comes near a hinge tie (|q - y| >= 1e-6), so a kernel whose q differs by
    rounding follows the same trajectory as the oracle;
  * FTRL: no step comes near the rescale threshold (|s²||θ||² - 1| >= 1e-9, 1000x the
    1e-12 band inside which the pipelined kernel's forms may decide differently), so regrets
    may be compared bit for bit between forms;
  * the family's own property (see each test).
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import _families as F

PIPE_DS = sorted({d for _, d in F.PIPE_SHAPES})


def test_case_list_covers_the_dispatched_shapes():
    from tests.test_gpu_pipe import SHAPES
    assert F.PIPE_SHAPES == SHAPES


def agrees_with_oracle(f, flag, tr):
    ref = O.simulate_alg_batch(f.z, f.y, flag, f.eta0, nthreads=4)[0]
    return np.all(np.abs(tr.regret - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref)))


def check_common(f, flag, tr, tie_ok=None):
    """The conditions every input meets.  tie_ok: [B, T] mask of steps built as exact ties
    (a zero row with a zero label: q - y = 0 - 0 in every arithmetic)."""
    assert agrees_with_oracle(f, flag, tr)
    m = tr.margin if tie_ok is None else tr.margin[~tie_ok]
    assert m.size == 0 or m.min() >= 1e-6
    if flag == 0 and tr.s2n.size:
        assert np.abs(tr.s2n - 1.0).min() >= 1e-9


def check_family(name, tr):
    if name == "straddle":
        assert 0.2 <= tr.rescaled.mean() <= 0.8
        assert F.mixed_share(tr.rescaled) >= 0.5
        # at least half of the sequences cross the threshold and come back
        flips = np.abs(np.diff(tr.rescaled.astype(np.int8), axis=1)).sum(axis=1)
        assert np.mean(flips >= 2) >= 0.5
    elif name == "always":
        assert tr.rescaled.mean() >= 0.95
    elif name == "small":
        assert 0.2 <= (tr.nth < 0.25).mean() <= 0.8
        # the hand-over between the re-sum and the running update is crossed mid-run
        assert np.all((tr.nth[:, 20:] < 0.25).any(axis=1))
    elif name == "pairs":
        assert np.all(tr.nth[:, ::2] == 0.0)
        assert np.all(tr.nth[:, 1::2] > 0.0)
    elif name == "gt_like":
        assert tr.rescaled.mean() <= 0.01   # the control: (almost) never rescales


@pytest.mark.parametrize("d", PIPE_DS)
@pytest.mark.parametrize("name", F.PIPE_FAMILIES)
def test_pipe_inputs(name, d):
    f = F.make(*F.pipe_case(name, d))
    tr = F.trace(f.z, f.y, f.flag, f.eta0)
    check_common(f, f.flag, tr)
    check_family(name, tr)


@pytest.mark.parametrize("case", F.SPLIT_CASES, ids=lambda c: f"{c[0]}-T{c[2]}-d{c[3]}")
def test_split_inputs(case):
    f = F.make(*case)
    tr = F.trace(f.z, f.y, 0, f.eta0)
    check_common(f, 0, tr)
    check_family(case[0], tr)


@pytest.mark.parametrize("d", PIPE_DS)
@pytest.mark.parametrize("name", F.SHORT_FAMILIES)
def test_short_horizon_inputs(name, d):
    """The family's conditions on the whole input (FTRL, its algorithm); the common ones on
    every prefix the GPU test runs, under FTRL and FTL."""
    f = F.make(*F.short_case(name, d))
    check_family(name, F.trace(f.z, f.y, 0, f.eta0))
    for T in F.SHORT_TS:
        p = F.Family(np.ascontiguousarray(f.z[:, :T]), np.ascontiguousarray(f.y[:, :T]), f.eta0, 0)
        for flag in (0, 1):
            tr = F.trace(p.z, p.y, flag, p.eta0)
            check_common(p, flag, tr)
            if T == 0:
                assert np.all(tr.regret == 0.0)


@pytest.mark.parametrize("d", sorted({d for _, d in F.CERT_SHAPES}))
def test_certificate_edge_inputs(d):
    f, edits, base = F.cert_case(d)
    assert (f.z != base.z).any(axis=(1, 2)).sum() + (f.y != base.y).any(axis=1).sum() == 11 + 1
    assert len(edits) == 11
    nrm = np.linalg.norm(f.z, axis=2)
    bad_row = nrm * nrm > 1.0 + 1e-12          # the kernels' row test
    bad_lab = np.abs(f.y) != 1.0
    tie_ok = (nrm == 0.0) & (f.y == 0.0)
    for b in range(F.CERT_B):                   # each violation is the only one in its sequence
        want = 1 if b in edits else 0
        assert bad_row[b].sum() + bad_lab[b].sum() == want, b
    for b, (kind, val, t) in edits.items():
        if kind == "row":
            assert bad_row[b, t] and abs(nrm[b, t] - val) <= 1e-15
        else:
            assert bad_lab[b, t] and f.y[b, t] == val
    for flag in (0, 1):
        tr = F.trace(f.z, f.y, flag, f.eta0)
        check_common(f, flag, tr, tie_ok)
        assert tr.margin[tie_ok].tolist() == [0.0]


@pytest.mark.parametrize("d", sorted({d for d, _ in F.RANGE_SHAPES}))
@pytest.mark.parametrize("name", F.RANGE_FAMILIES)
def test_range_inputs(name, d):
    f = F.range_case(name, d)
    tr = F.trace(f.z, f.y, 0, f.eta0)
    check_common(f, 0, tr)
    check_family(name, tr)
    nrm = np.linalg.norm(f.z, axis=2)
    unclean = np.nonzero((nrm * nrm > 1.0 + 1e-12).any(axis=1) | (np.abs(f.y) != 1.0).any(axis=1))[0]
    assert tuple(unclean) == F.RANGE_UNCLEAN
    assert tr.regret.max() > 0.0    # the folded maximum is a regret, not the 0.0 it starts from
