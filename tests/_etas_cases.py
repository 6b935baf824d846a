"""Inputs of the step-size sweep tests (tests/test_gpu_etas.py, tests/test_etas_cpu.py).

On the suite's usual rows every step size has the same θ trajectory: the rows lie in the unit
ball and the labels are ±1, so |q| <= 1 and every sub-gradient is -y/2 whatever eta0 is.  A
sweep kernel that shared θ across its columns would pass on them.  The `beam` family makes the
trajectories differ in every sequence: its rows are 1.6 s u + 0.3 n (u a fixed unit direction
per sequence, s = ±1, n a unit noise row), of norm about 1.6, so |q| exceeds 1 once the action
is long enough, the sub-gradient's sign then depends on the step size, and θ with it.

`sign_trace` follows fast_algorithms.py:88-115 in NumPy float64 and records, per step and
sequence, the sub-gradient's sign and whether FTRL rescaled its action.  It is a diagnostic
for choosing inputs (tests/test_etas_cpu.py asserts the conditions), not a parity reference:
that stays the C oracle and the existing kernels.
"""
import math

import numpy as np

from tests import _families as F

SQ2 = math.sqrt(2.0)
B, T = 24, 257
ETAS = (0.25, 1.0, SQ2, 2.0, 8.0)
# unsorted, with a duplicate, and a tail group of 7 mod 4 = 3
ETAS7 = [8.0, 0.25, SQ2, SQ2, 1.0, 2.0, 4.0 * SQ2]
# every dimension the GPU tests run `beam` at
DIMS = (5, 16, 32, 64, 100, 128, 256, 512, 1024)


def beam(d, B=B, T=T):
    """The `beam` family at dimension d: a Family with eta0 = sqrt 2 (the sweeps pass their
    own step sizes) and flag 0."""
    rng = np.random.default_rng(4000 + d)
    u = rng.standard_normal((B, 1, d))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    s = np.where(rng.random((B, T, 1)) < 0.5, -1.0, 1.0)
    n = rng.standard_normal((B, T, d))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    z = 1.6 * s * u + 0.3 * n
    y = np.where(rng.random((B, T)) < 0.5, -1.0, 1.0)
    return F.Family(np.ascontiguousarray(z), y, SQ2, 0)


def sign_trace(z, y, eta0):
    """FTRL (fast_algorithms.py:88-115) in NumPy float64, every sequence at once: the
    sub-gradient signs [B, T] (-1, 0, 1) and whether the action was rescaled [B, T]."""
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    Bn, Tn, d = z.shape
    theta = np.zeros((Bn, d))
    signs = np.zeros((Bn, Tn))
    rescaled = np.zeros((Bn, Tn), dtype=bool)
    for t in range(Tn):
        x = -(eta0 / math.sqrt(t + 1)) * theta
        n2 = np.sum(x * x, axis=1)
        rescaled[:, t] = n2 > 1.0
        x = np.where(rescaled[:, t, None], x * (1.0 / np.sqrt(np.maximum(n2, 1.0)))[:, None], x)
        diff = np.sum(z[:, t] * x, axis=1) - y[:, t]
        signs[:, t] = np.sign(diff)
        theta += (0.5 * signs[:, t])[:, None] * z[:, t]
    return signs, rescaled


def cert_etas_case(d):
    """F.cert_case(d) with two further sequences (2 and 22: each shares a wave-group with
    unedited sequences in every layout of F.CERT_SHAPES with more than one sequence per wave)
    whose rows 0 and 1 are e_1 with labels +1.  In the reference's order step 1 then plays
    x = 0.5 e_1 at eta0 = sqrt 2 (a strict margin: the certificate holds) and exactly 1.0 e_1
    at eta0 = 4 sqrt 2 (q - y = 0: the sub-gradient is 0 and the certificate breaks); every
    factor is a power of two.  Returns (Family, F.cert_case's edits, the two sequences)."""
    f, edits, _ = F.cert_case(d)
    z, y = f.z.copy(), f.y.copy()
    two = (2, 22)
    for b in two:
        assert b not in edits
        z[b, 0:2] = 0.0
        z[b, 0:2, 0] = 1.0
        y[b, 0:2] = 1.0
    return F.Family(z, y, f.eta0, f.flag), edits, two


CERT_ETAS = (SQ2, 4.0 * SQ2, 1.0)
