"""Inputs of the SMART regret-curve tests (tests/test_gpu_smart_curve.py,
tests/test_smart_curve_cpu.py): the families, shapes and dimensions of the threshold sweep
tests (tests/_thresholds_cases.py) with seven (horizon, threshold) pairs.

On `gt_like` rows the switch at threshold th falls near t ≈ 4·th², so each MID pair's horizon
(36 with 3, 100 with 6, 144 with 7, 64 with 4 — roughly 4·th² each) cuts its column's
switch-step distribution in half: some sequences have switched before t_k, others would switch
later and must report -1 and FTL's loss so far.  A kernel that ignored the horizon, or froze a
column late, cannot pass.  Column 0 (-1) switches at step 0 everywhere, column 3 (+inf) is FTL
at horizon 100, and 7 mod 4 = 3 gives a tail group.  tests/test_smart_curve_cpu.py asserts the
conditions with the C oracle."""
import functools
import math

import numpy as np

from tests import _thresholds_cases as TC

family, B, T, DIMS, FAMILIES, SQ2 = TC.family, TC.B, TC.T, TC.DIMS, TC.FAMILIES, TC.SQ2

CK7 = [1, 36, 64, 100, 144, 196, 257]
TH7C = [-1.0, 3.0, 4.0, math.inf, 6.0, 7.0, 8.0]     # 7 mod 4 = 3: a tail group
MID = (1, 2, 4, 5)
INF_COL = 3
assert CK7[-1] == T and len(CK7) == len(TH7C)


@functools.lru_cache(maxsize=None)
def oracle_curve(name, d):
    """(regret [B, 7], switch_step [B, 7]) of the C oracle's SMART on the rows truncated at
    CK7[k] with threshold TH7C[k], one run per column.  Shared between tests: never written
    to."""
    from oracle import oracle as O
    f = family(name, d)
    cols = [O.simulate_smart_batch(np.ascontiguousarray(f.z[:, :t]),
                                   np.ascontiguousarray(f.y[:, :t]), np.full(B, th), SQ2,
                                   nthreads=4) for t, th in zip(CK7, TH7C)]
    return (np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1))


@functools.lru_cache(maxsize=None)
def oracle_full(name, d):
    """switch_step [B, 7] of the C oracle's SMART on the whole rows with TH7C's thresholds."""
    from oracle import oracle as O
    f = family(name, d)
    return np.stack([O.simulate_smart_batch(f.z, f.y, np.full(B, th), SQ2, nthreads=4)[1]
                     for th in TH7C], axis=1)


def pre_switch_steps(sw, horizons):
    """Steps a column spends before its switch, the switch step included: its horizon where it
    never switches (-1), sw + 1 otherwise.  sw [B, K], horizons [K]."""
    sw = np.asarray(sw)
    return np.where(sw < 0, np.asarray(horizons)[None, :], sw + 1)
