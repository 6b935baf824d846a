"""The inputs of the twin column tests do what tests/test_gpu_twin32_cols.py needs, and the host
side of engine.twin32_cols_batch validates its lists (NumPy and the oracle only, no GPU).

With oracle.t32_simulate_smart_full on the full sequences: at every dimension of the cases file
and in every MID column, at least 13 sequences have switched before the column's horizon and at
least 2 switch at or after it in the full run (at least 40 summed over MID), and the +inf column
never switches — so a kernel that ignored or misplaced a horizon cannot pass.  The bounds are the
oracle's own minima (d = 1: 13 before; d = 8: 2 later; d = 16: 41 summed); a change
of CK7 or TH7 re-derives them from the oracle, never from the kernel."""
import os

import numpy as np
import pytest

from online_convex_optimization_amd import engine
from tests import _twin32_cols_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("d", C.DIMS)
def test_mid_horizons_cut_the_switch_steps_in_two(d):
    full = C.oracle_full_switch(d)
    hz = np.array(C.CK7)
    before = ((full >= 0) & (full < hz[None, :])).sum(axis=0)
    later = (full >= hz[None, :]).sum(axis=0)
    print("switched before / at or after t_k", d, before.tolist(), later.tolist())
    mid = list(C.MID)
    assert before[mid].min() >= 13, (d, before)
    assert later[mid].min() >= 2, (d, later)
    assert later[mid].sum() >= 40, (d, later)
    assert np.all(full[:, C.INF_COL] == -1) and C.TH7[C.INF_COL] == np.inf


def test_golden_smart_fixture_is_split_by_the_cut_horizons():
    """tests/golden/twin32.npz: threshold 2 at horizon 30 has 4 sequences switched and 3 that
    switch later; threshold 5 at horizon 75 has 3 and 2."""
    with np.load(os.path.join(HERE, "golden", "twin32.npz"), allow_pickle=False) as f:
        th, sw = f["smart_thresh"], f["smart_sw"]
    for want_th, h, nb, nl in ((2.0, 30, 4, 3), (5.0, 75, 3, 2)):
        i = list(th).index(want_th)
        assert ((sw[i] >= 0) & (sw[i] < h)).sum() == nb
        assert (sw[i] >= h).sum() == nl


def test_algos_argument_is_validated_on_the_host():
    a = engine._twin32_algos(2, 3)
    assert a.dtype == np.int32 and a.tolist() == [2, 2, 2]
    assert engine._twin32_algos("FTL", 2).tolist() == [1, 1]
    assert engine._twin32_algos(["FTRL", 1, "SMART", np.int64(0)], 4).tolist() == [0, 1, 2, 0]
    assert engine._twin32_algos(np.array([2, 1, 0]), 3).tolist() == [2, 1, 0]
    assert engine._twin32_algos([], 0).shape == (0,)
    assert engine._twin32_algos(C.MIX_ALGO, 9).tolist() == [C.ALGO_CODE[a] for a in C.MIX_ALGO]
    for bad, K in (("EMP", 2), (["FTRL", "ftl"], 2), (3, 1), (-1, 1), ([0, 1], 3), ([0, 1, 2], 2),
                   (True, 1), ([True, False], 2), (1.0, 1), ([1.5], 1), (None, 1), ([None], 1),
                   ([[0, 1]], 1)):
        with pytest.raises(ValueError):
            engine._twin32_algos(bad, K)


def test_thresholds_argument_is_validated_on_the_host():
    hz = np.array([4, 4, 9], dtype=np.int64)
    al = np.array([0, 2, 2], dtype=np.int32)
    B = 3
    # None: sqrt(2 t_k) in the SMART columns
    th = engine._twin32_cols_thresholds(None, hz, al, B)
    assert th.shape == (B, 3) and th.dtype == np.float64 and th.flags["C_CONTIGUOUS"]
    assert np.array_equal(th[:, 1], np.full(B, np.sqrt(8.0)))
    assert np.array_equal(th[:, 2], np.full(B, np.sqrt(18.0)))
    # no SMART column: no thresholds at all, whatever was passed
    assert engine._twin32_cols_thresholds(None, hz, np.array([0, 1, 1], dtype=np.int32), B) is None
    assert engine._twin32_cols_thresholds([np.nan] * 3, hz, np.array([0, 1, 0], dtype=np.int32),
                                          B) is None
    # [K] and [B, K]; NaN fills the FTRL / FTL columns; +-inf are legal thresholds
    th = engine._twin32_cols_thresholds([np.nan, 2.0, np.inf], hz, al, B)
    assert np.array_equal(th[:, 1:], np.tile([2.0, np.inf], (B, 1))) and not np.isnan(th).any()
    per = np.arange(9.0).reshape(B, 3)
    assert np.array_equal(engine._twin32_cols_thresholds(per, hz, al, B)[:, 1:], per[:, 1:])
    z = np.zeros((B, 9, 2), dtype=np.float32)
    y = np.ones((B, 9), dtype=np.float32)
    for bad in ([1.0, 2.0], [1.0, 2.0, 3.0, 4.0], np.zeros((B + 1, 3)), np.zeros((2, 2, 3)),
                ["a", "b", "c"], [np.nan, np.nan, 1.0], [np.nan, 1.0, np.nan],
                np.where(np.eye(3) > 0, np.nan, 1.0), 1.0):
        with pytest.raises(ValueError):
            engine._twin32_cols_thresholds(bad, hz, al, B)
        with pytest.raises(ValueError):  # the public call validates before it loads the library
            engine.twin32_cols_batch(z, y, hz, al, bad)
    for bad_algos in ("EMP", [0, 2], [0, 1, 3]):
        with pytest.raises(ValueError):
            engine.twin32_cols_batch(z, y, hz, bad_algos)
    for bad_hz in ([9, 4, 4], [0, 4, 10], [1.5, 2, 3]):
        with pytest.raises(ValueError):
            engine.twin32_cols_batch(z, y, bad_hz, al)
