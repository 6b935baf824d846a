"""Inputs of the threshold sweep tests (tests/test_gpu_thresholds.py,
tests/test_thresholds_cpu.py).

A sweep kernel that shared the switch step or the FTRL state between its columns would pass
on inputs where every threshold switches at the same step.  TH7 spreads the switches of every
sequence of both families over the horizon (tests/test_thresholds_cpu.py asserts it with the
C oracle): it is unsorted, holds a duplicate and an FTL column (+inf never switches), and
7 mod 4 = 3 gives a tail group.  The `beam` rows (tests/_etas_cases.py) lie outside the unit
ball, so the closed-form prefix never applies to them and every pre-switch step re-scans.
"""
import functools
import math

import numpy as np

from tests import _etas_cases as E
from tests import _families as F

SQ2 = math.sqrt(2.0)
B, T = E.B, E.T   # 24, 257
TH7 = [3.0, -1.0, 0.75, 0.75, math.inf, 1.5, 5.0]
INF_COL = 4
DUP_COLS = (2, 3)
# every dimension the GPU tests run the two families at
DIMS = (5, 16, 32, 64, 100, 128, 256, 512, 1024)
FAMILIES = ("beam", "gt_like")

# the guard-band case: half-integer thresholds meet the flip sequence's half-integer
# ftl_loss - s_loss exactly
FLIP_T = 400
FLIP_TH = np.arange(-2.0, 40.0, 0.5)   # 84 columns


@functools.lru_cache(maxsize=None)
def family(name, d):
    """Shared between tests: never written to."""
    if name == "beam":
        return E.beam(d)
    return F.make(name, B, T, d, 100 + d)


@functools.lru_cache(maxsize=None)
def oracle_columns(name, d):
    """(regret [B, 7], switch_step [B, 7]) of the C oracle's SMART, one run per column of TH7.
    Shared between tests: never written to."""
    from oracle import oracle as O
    f = family(name, d)
    cols = [O.simulate_smart_batch(f.z, f.y, np.full(B, th), SQ2, nthreads=4) for th in TH7]
    return (np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1))


def pre_switch_steps(sw, T):
    """Steps a column spends before its switch, the switch step included: T where it never
    switches (-1), sw + 1 otherwise."""
    sw = np.asarray(sw)
    return np.where(sw < 0, T, sw + 1)
