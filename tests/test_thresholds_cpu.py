"""The inputs of the threshold sweep tests do what tests/test_gpu_thresholds.py needs (NumPy and
the C oracle only): on every sequence of both families, at every dimension the GPU tests use,
TH7's columns switch at spread-out steps, so a kernel that shared the switch step or the FTRL
state between its columns cannot pass; the +inf column is FTL; the flip sequence meets 84
half-integer thresholds at many different steps."""
import numpy as np
import pytest

from oracle import oracle as O
from online_convex_optimization_amd.engine import _thresholds
from tests import _thresholds_cases as C


def test_thresholds_argument_is_validated_on_the_host():
    """[M] broadcasts to [B, M]; [B, M] passes through; NaN and ±inf are legal; anything that
    is not one or two dimensions of real numbers, or has the wrong B, is a ValueError."""
    a = _thresholds(C.TH7, 3)
    assert a.shape == (3, 7) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    assert np.array_equal(a, np.tile(np.array(C.TH7), (3, 1)))
    per = np.arange(6.0).reshape(3, 2)
    assert np.array_equal(_thresholds(per, 3), per)
    assert _thresholds([], 3).shape == (3, 0)
    odd = _thresholds([np.nan, np.inf, -np.inf, 1], 2)
    assert np.isnan(odd[1, 0]) and odd[1, 1] == np.inf and odd[0, 2] == -np.inf
    for bad in (np.zeros((3, 2, 1)), ["a", "b"], None, [None], [1.0 + 2.0j], 1.0,
                np.zeros((4, 2)), [[1.0, 2.0], [3.0]]):
        with pytest.raises(ValueError):
            _thresholds(bad, 3)


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("d", C.DIMS)
def test_th7_spreads_the_switches_of_every_sequence(name, d):
    f = C.family(name, d)
    reg, sw = C.oracle_columns(name, d)
    assert reg.shape == sw.shape == (C.B, len(C.TH7))
    distinct = np.array([len(set(row.tolist())) for row in sw])
    assert distinct.min() >= 4, (name, d, distinct.min())
    assert distinct.mean() >= 5.5, (name, d, distinct.mean())
    # the +inf column never switches and is FTL's regret, bit for bit
    assert np.all(sw[:, C.INF_COL] == -1)
    ftl = O.simulate_alg_batch(f.z, f.y, 1, C.SQ2, nthreads=4)[0]
    assert np.array_equal(reg[:, C.INF_COL], ftl), (name, d)
    # six distinct regret columns (the duplicate threshold gives the seventh)
    cols = {reg[:, m].tobytes() for m in range(len(C.TH7))}
    assert len(cols) == 6, (name, d, len(cols))
    assert np.array_equal(reg[:, C.DUP_COLS[0]], reg[:, C.DUP_COLS[1]])
    assert np.array_equal(sw[:, C.DUP_COLS[0]], sw[:, C.DUP_COLS[1]])


def test_flip_sequence_switches_in_every_column_at_many_steps():
    z, y, _ = O.flip_sequence(C.FLIP_T)
    th = C.FLIP_TH
    assert len(th) == 84
    Z = np.repeat(z[None].astype(np.float64), len(th), axis=0)
    Y = np.repeat(y[None].astype(np.float64), len(th), axis=0)
    _, sw = O.simulate_smart_batch(Z, Y, th, C.SQ2, nthreads=4)
    assert np.all(sw >= 0)
    assert len(set(sw.tolist())) >= 70, len(set(sw.tolist()))
