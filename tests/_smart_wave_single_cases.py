"""Inputs of the single-threshold wave test (tests/test_gpu_smart_wave_cols.py
test_single_call_equals_the_oracle; conditions asserted in tests/test_smart_wave_cols_cpu.py).

The single call under OCX_SMART_KERNEL=wave runs ocx_smart_wave_kernel whatever the layout.
DIMS are the two sides of its row-path split (d <= 8 keeps a chunk's rows in registers).  HORIZONS: 1 and 3 are shorter than one group of four speculated steps, 64 is one
LDS chunk of the prefix scan exactly, 67 a chunk plus a partial group (steps 64, 65, 66).  B is
no multiple of the four waves of a block.  Every horizon runs the first T rows of the same
`gt_like` rows with the same per-sequence thresholds: on those rows the switch at threshold th
falls near 4·th², so thresholds up to 4.6 spread the switches over the 67 steps and past them.
SEED was chosen with the C oracle alone so that at T = 67 the switch steps hit every position
of a speculated group, the last group and -1."""
import functools

import numpy as np

from tests import _families as F
from tests import _thresholds_cases as TC

SQ2 = TC.SQ2
DIMS = (8, 9)
HORIZONS = (1, 3, 64, 67)
LAYOUTS = (1, -1, -4, 8)   # 8: a butterfly layout, which the single call also takes in wave form
B, TMAX = 38, HORIZONS[-1]
SEED = 2
assert B % 4 and TMAX == max(HORIZONS)


@functools.lru_cache(maxsize=None)
def inputs(d):
    """(z [B, TMAX, d], y [B, TMAX], thresholds [B]).  Shared between tests: never written
    to."""
    f = F.make("gt_like", B, TMAX, d, SEED + d)
    th = np.random.default_rng(SEED + 1000 + d).uniform(-0.2, 4.6, size=B)
    return f.z, f.y, th


@functools.lru_cache(maxsize=None)
def oracle(d, T):
    """(regret [B], switch_step [B]) of the C oracle's SMART on the first T rows.  Shared
    between tests: never written to."""
    from oracle import oracle as O
    z, y, th = inputs(d)
    return O.simulate_smart_batch(np.ascontiguousarray(z[:, :T]), np.ascontiguousarray(y[:, :T]),
                                  th.copy(), SQ2, nthreads=4)
