"""Inputs of the SMART regret-grid tests (tests/test_gpu_smart_grid.py,
tests/test_smart_grid_cpu.py): the families, shapes and dimensions of the threshold sweep tests
(tests/_thresholds_cases.py) with M thresholds observed at K checkpoints.

On `gt_like` rows the switch at threshold th falls near t ≈ 4·th², so at each interior
checkpoint of CK7 some columns of THG7 have all switched, some none, and one is split: some
sequences have switched before t_k, the others switch later and must report -1 and FTL's loss
so far at t_k, their own step and total at a later checkpoint.  A kernel that emits the final
switch step early, or a column's own total before its switch, cannot pass.  THG7 is unsorted,
holds a duplicate (3.0) and an FTL column (+inf), and 7 mod 4 = 3 gives a tail group.

HZ9 x THG9 are the one-wave-per-sequence form's: 9 mod 8 = 1 (a tail launch of one column), and
the checkpoints sit inside a group of four speculated steps (2, 3; 65, 66) and on both sides of
a 64-row chunk (63, 65).  tests/test_smart_grid_cpu.py asserts the conditions with the C
oracle."""
import functools
import math

import numpy as np

from tests import _thresholds_cases as TC

family, B, T, DIMS, FAMILIES, SQ2 = TC.family, TC.B, TC.T, TC.DIMS, TC.FAMILIES, TC.SQ2

CK7 = [1, 36, 64, 100, 144, 196, 257]
THG7 = [4.0, -1.0, 7.0, 3.0, math.inf, 3.0, 6.0]
SPLIT_TH = (3.0, 4.0, 6.0, 7.0)
INF_COL = 4
DUP_COLS = (3, 5)

HZ9 = [0, 2, 3, 63, 65, 66, 130, 255, 257]
THG9 = [4.0, -1.0, 0.5, 8.0, math.inf, 0.25, 5.7, 4.0, 2.0]
WAVE_DIMS = (1, 5, 8, 9, 16, 64)
assert CK7[-1] == T and HZ9[-1] == T


def _trunc(a, t):
    return np.ascontiguousarray(a[:, :t])


@functools.lru_cache(maxsize=None)
def oracle_full(name, d, ths):
    """(regret [B, M], switch_step [B, M]) of the C oracle's SMART on the whole rows, one run
    per threshold of the tuple `ths`.  Shared between tests: never written to."""
    from oracle import oracle as O
    f = family(name, d)
    cols = [O.simulate_smart_batch(f.z, f.y, np.full(B, th), SQ2, nthreads=4) for th in ths]
    return (np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1))


@functools.lru_cache(maxsize=None)
def oracle_grid(name, d, ck, ths):
    """(regret [B, M, K], switch_step [B, M, K]) of the C oracle's SMART: one run per
    (threshold, checkpoint) on the rows truncated at the checkpoint.  `ck` and `ths` are
    tuples.  Shared between tests: never written to."""
    from oracle import oracle as O
    f = family(name, d)
    reg = np.zeros((B, len(ths), len(ck)))
    sw = np.zeros((B, len(ths), len(ck)), dtype=np.int64)
    for k, t in enumerate(ck):
        z, y = _trunc(f.z, t), _trunc(f.y, t)
        for m, th in enumerate(ths):
            reg[:, m, k], sw[:, m, k] = O.simulate_smart_batch(z, y, np.full(B, th), SQ2,
                                                               nthreads=4)[:2]
    return reg, sw


def truncate_switch(full_sw, ck):
    """[B, M, K] from the full run's switch steps [B, M]: the step where it lies before t_k,
    else -1."""
    full_sw = np.asarray(full_sw)[:, :, None]
    t = np.asarray(ck)[None, None, :]
    return np.where((full_sw >= 0) & (full_sw < t), full_sw, -1)


def pre_switch_steps(full_sw, t_last):
    """Steps a column spends before its switch, the switch step included, capped at the last
    checkpoint: t_last where it does not switch before it, sw + 1 otherwise."""
    full_sw = np.asarray(full_sw)
    return np.where((full_sw < 0) | (full_sw >= t_last), t_last, full_sw + 1)


def pairs(ck, ths):
    """The grid as simulate_smart_curve's pair list sorted by horizon: (horizons [K·M],
    thresholds [K·M]) with pair k·M + m = (ck[k], ths[m])."""
    M = len(ths)
    return [t for t in ck for _ in range(M)], [th for _ in ck for th in ths]
