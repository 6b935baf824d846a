"""Inputs of the FTRL-vs-exact-FTL regret-grid tests (tests/test_gpu_exact_grid.py,
tests/test_exact_grid_cpu.py): the checkpoint lists of tests/test_gpu_exact_curve.py (ring
depth, the 64-step boundaries of the FTRL scale table, both ends), the step sizes of
tests/_etas_cases.py (unsorted, one duplicate, a tail of 3 for group 4 and of 1 for group 2),
and the families, each built once and never written to.

On the suite's usual rows every step size has the same θ_r trajectory; `beam`
(tests/_etas_cases.py) makes the trajectories and the rescale decisions differ between the
columns in every sequence — tests/test_exact_grid_cpu.py asserts both at every dimension the GPU
tests use — and its rows, of norm about 1.6, lie outside the l2 regime, so every pair streams.
"""
import functools

import numpy as np

from tests import _etas_cases as E
from tests import _families as F

B, T = 24, 257
CHECKPOINTS = [0, 1, 2, 63, 64, 65, 128, 129, 256, 257]
SHORT_B, SHORT_T = 6, 40
SHORT_CHECKPOINTS = [0, 1, 2, 7, 8, 9, 39, 40]
CERT_CHECKPOINTS = [0, 1, 63, 64, 65, 129, 130]
ETAS7 = list(E.ETAS7)
SQ2 = E.SQ2

# every layout class of the curve tests: (lanes_per_seq, d)
LAYOUTS = list(F.PIPE_SHAPES) + [(0, 5), (0, 64), (128, 5), (128, 64), (1, 64), (-4, 64)]
# the exact modes of the oracle test
EXACT = [(P, d) for d in (5, 16, 64) for P in (1, -1, -4)]
# every dimension at which a GPU test runs `beam`
BEAM_DIMS = sorted({d for _, d in LAYOUTS if d in E.DIMS} | {5, 16, 64})


@functools.lru_cache(maxsize=None)
def family(name, d, B=B, T=T, norm="l2"):
    """Family `name` (tests/_families.py, or `beam`) at [B, T, d].  linf: rows scaled into the
    dual ball (||z||_1 <= 1), as tests/test_gpu_exact_curve.py's `family` does, so every prefix
    is in the closed form's regime (l1: gt_like rows have ||z||_inf <= 1 already)."""
    f = E.beam(d, B, T) if name == "beam" else F.make(name, B, T, d, 100 + d)
    if norm == "linf":
        z = f.z / np.maximum(1.0, np.abs(f.z).sum(axis=2, keepdims=True))
        f = F.Family(z, f.y, f.eta0, f.flag)
    return f


def families_for(d):
    """The l2 families of the every-layout test at dimension d."""
    return ("gt_like", "straddle", "always") + (("beam",) if d in E.DIMS else ())
