"""Inputs of the one-wave-per-sequence sweep tests (tests/test_gpu_smart_wave_cols.py,
tests/test_smart_wave_cols_cpu.py) beyond those of tests/_thresholds_cases.py and
tests/_smart_curve_cases.py, which they reuse.

DIMS covers the kernel's two row paths (d <= 8 keeps a chunk's rows in registers, d > 8 reads
them as it goes), their boundary (8, 9), one coordinate, and a wave in which every lane owns a
coordinate (64).

HZ9 puts horizons where the kernel's own structure has edges: inside a group of four
speculated steps (2, 3; 65, 66 after a group that starts at 64), on both sides of a 64-row
chunk of the prefix scan (63, 65), and at rows 130, 255 and T = 257.  TH9 follows
tests/_smart_curve_cases.py: on `gt_like` rows the switch at threshold th falls near 4·th², so
each MID9 column's horizon cuts its switch steps in two (asserted with the C oracle in
tests/test_smart_wave_cols_cpu.py).  Column 0 is the empty run, column 8 (+inf) FTL on the
whole rows."""
import functools
import math

import numpy as np

from tests import _thresholds_cases as TC

family, B, T, FAMILIES, SQ2 = TC.family, TC.B, TC.T, TC.FAMILIES, TC.SQ2

DIMS = (1, 5, 8, 9, 16, 64)
HZ9 = [0, 2, 3, 63, 65, 66, 130, 255, 257]
TH9 = [-1.0, 0.25, 0.5, 4.0, 4.0, 4.0, 5.7, 8.0, math.inf]
MID9 = (3, 4, 5, 6, 7)
assert HZ9[-1] == T and len(HZ9) == len(TH9)


@functools.lru_cache(maxsize=None)
def oracle_curve9(name, d):
    """(regret [B, 9], switch_step [B, 9]) of the C oracle's SMART on the rows truncated at
    HZ9[k] with threshold TH9[k], one run per column.  Shared between tests: never written
    to."""
    from oracle import oracle as O
    f = family(name, d)
    cols = [O.simulate_smart_batch(np.ascontiguousarray(f.z[:, :t]),
                                   np.ascontiguousarray(f.y[:, :t]), np.full(B, th), SQ2,
                                   nthreads=4) for t, th in zip(HZ9, TH9)]
    return (np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1))
