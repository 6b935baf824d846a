"""Input families that drive the FTRL/FTL kernels into the branches g(T)-like rows never
take, a plain NumPy float64 step trace that shows they do, and the case lists that
tests/test_families_cpu.py (the trace's conditions) and tests/test_gpu_alg_branches.py (the
kernels against the C oracle) share.

The trace follows fast_algorithms.py:88-115 step by step.  It is a diagnostic for choosing
inputs — which steps rescale, how close a step comes to a branch's threshold or to a hinge
tie — and not a parity reference: that stays the C oracle (oracle/ocx_oracle.c).

Families (rows dense with norm <= 1, labels ±1):
  gt_like   normal rows clipped to the ball, eta0 = sqrt 2: the suite's usual recipe (control).
            s²||θ||² stays near 0.5, so FTRL never rescales.
  straddle  random unit rows, eta0 = 2: s²||θ||² hovers about 1, so FTRL rescales on roughly
            half of the steps, sequences cross the threshold back and forth, and a wave
            holds rescaled and unrescaled sequences at once.
  always    the same rows, eta0 = 8: FTRL rescales on nearly every step.
  pairs     z_{2k+1} = z_{2k}, y_{2k+1} = -y_{2k}, row norms in [0.3, 0.99] (FTL): θ returns to
            exactly 0 after every pair, so FTL's q = 0 branch runs at every even step.
  small     rows of norm 0.1 (FTL): ||θ||² crosses 0.25, the bound below which the pipelined
            kernel sums ||θ||² afresh, in the middle of the run and sequence by sequence.
"""
import math
from collections import namedtuple

import numpy as np

SQ2 = math.sqrt(2.0)

# z [B, T, d], y [B, T], the FTRL step size, the algorithm the family is built for (0 FTRL, 1 FTL)
Family = namedtuple("Family", "z y eta0 flag")
ETA0 = {"gt_like": SQ2, "straddle": 2.0, "always": 8.0, "pairs": SQ2, "small": SQ2}
FLAG = {"gt_like": 0, "straddle": 0, "always": 0, "pairs": 1, "small": 1}


def _labels(rng, B, T):
    return np.where(rng.random((B, T)) < 0.5, -1.0, 1.0)


def make(name, B, T, d, seed):
    """Family `name` at shape (B, T, d) from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    if name == "pairs":
        H = (T + 1) // 2
        zh = rng.standard_normal((B, H, d))
        zh *= rng.uniform(0.3, 0.99, (B, H, 1)) / np.linalg.norm(zh, axis=2, keepdims=True)
        yh = _labels(rng, B, H)
        z = np.repeat(zh, 2, axis=1)[:, :T]
        y = np.stack([yh, -yh], axis=2).reshape(B, 2 * H)[:, :T]
        return Family(np.ascontiguousarray(z), np.ascontiguousarray(y), ETA0[name], FLAG[name])
    z = rng.standard_normal((B, T, d))
    nrm = np.linalg.norm(z, axis=2, keepdims=True)
    if name == "gt_like":
        z /= np.maximum(1.0, nrm)
    elif name in ("straddle", "always"):
        z /= np.where(nrm > 0.0, nrm, 1.0)
    elif name == "small":
        z *= 0.1 / np.where(nrm > 0.0, nrm, 1.0)
    else:
        raise KeyError(name)
    return Family(z, _labels(rng, B, T), ETA0[name], FLAG[name])


Trace = namedtuple("Trace", "rescaled s2n nth margin regret")


def trace(z, y, flag, eta0):
    """fast_algorithms.py:88-115 in NumPy float64, every sequence of z [B, T, d] at once.
    Per step and sequence ([B, T]): whether FTRL rescaled its action, s²||θ_t||² (FTRL; NaN
    for FTL), ||θ_t||², |q_t - y_t|; and the regret [B]."""
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    B, T, d = z.shape
    theta = np.zeros((B, d))
    cum = np.zeros(B)
    rescaled = np.zeros((B, T), dtype=bool)
    s2n = np.full((B, T), np.nan)
    nth = np.zeros((B, T))
    margin = np.zeros((B, T))

    def ftl(th):
        n2 = np.sum(th * th, axis=1)
        sc = np.where(n2 == 0.0, 0.0, -(1.0 / np.sqrt(np.where(n2 == 0.0, 1.0, n2))))
        return sc[:, None] * th

    for t in range(T):
        nth[:, t] = np.sum(theta * theta, axis=1)
        if flag == 0:
            x = -(eta0 / math.sqrt(t + 1)) * theta
            n2 = np.sum(x * x, axis=1)
            s2n[:, t] = n2
            rescaled[:, t] = n2 > 1.0
            x = np.where(rescaled[:, t, None], x * (1.0 / np.sqrt(np.maximum(n2, 1.0)))[:, None], x)
        else:
            x = ftl(theta)
        diff = np.sum(z[:, t] * x, axis=1) - y[:, t]
        margin[:, t] = np.abs(diff)
        cum += 0.5 * margin[:, t]
        theta += (0.5 * np.sign(diff))[:, None] * z[:, t]
    xs = ftl(theta)
    comp = np.zeros(B)
    for t in range(T):
        comp += 0.5 * np.abs(np.sum(z[:, t] * xs, axis=1) - y[:, t])
    return Trace(rescaled, s2n, nth, margin, cum - comp)


def mixed_share(rescaled):
    """Share of (group of 8 neighbouring sequences, step) pairs that hold both a rescaled and
    an unrescaled sequence: what a wave of the 8-lane layouts sees in one step."""
    B = rescaled.shape[0]
    both = [rescaled[g:g + 8].any(axis=0) & ~rescaled[g:g + 8].all(axis=0)
            for g in range(0, B, 8) if min(B, g + 8) - g >= 2]
    return float(np.mean(both))


# ----------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_alg_branches.py.  test_families_cpu.py walks the same lists.
# ----------------------------------------------------------------------------------------
# the pipelined kernel's dispatched shapes (tests/test_gpu_pipe.py SHAPES): (lanes, d)
PIPE_SHAPES = [(8, 32), (8, 64), (8, 128), (8, 256), (16, 64), (16, 128), (16, 512), (32, 128),
               (32, 1024), (64, 1024)]
PIPE_B = 24


def pipe_case(name, d):
    """(family, B, T, d, seed) of the pipelined-kernel test for one family and dimension."""
    if name in ("straddle", "always"):
        return name, PIPE_B, 200, d, d
    return name, PIPE_B, 257, d, 100 + d


PIPE_FAMILIES = ("straddle", "always", "pairs", "small")

# the plain kernel, every lane split: (family, B, T, d, seed)
SPLIT_B = 37
SPLIT_CASES = [(name, SPLIT_B, T, d, 7000 + d) for name in ("straddle", "always")
               for T, d in ((120, 16), (96, 64), (64, 100))]

# short horizons: every T below is a prefix of one input of SHORT_TMAX steps (the trace of a
# prefix is the prefix of the trace)
SHORT_TS = list(range(0, 21)) + [63, 64, 65, 127, 128, 129]
SHORT_TMAX = 129
SHORT_B = 21
SHORT_FAMILIES = ("gt_like", "straddle")


def short_case(name, d):
    return name, SHORT_B, SHORT_TMAX, d, 300 + d


# certificate edges at pipelined shapes
CERT_SHAPES = [(8, 64), (16, 64), (32, 128), (64, 1024)]
CERT_B, CERT_T = 37, 130


def cert_case(d):
    """gt_like rows with eleven sequences that each break the closed form's certificate in
    exactly one place.  Returns (Family, {sequence: what was done to it}, the rows before the
    edits)."""
    T = CERT_T
    f = make("gt_like", CERT_B, T, d, 500 + d)
    z, y = f.z.copy(), f.y.copy()
    edits = {}
    seqs = iter((1, 4, 9, 12, 17, 20, 25, 28, 30, 33, 36))
    for scale in (1.5, 1.0 + 1e-9):
        for t in (0, 63, 64, T - 1):
            b = next(seqs)
            z[b, t] *= scale / np.linalg.norm(z[b, t])
            edits[b] = ("row", scale, t)
    for t in (0, T - 1):
        b = next(seqs)
        y[b, t] = 0.5
        edits[b] = ("label", 0.5, t)
    b = next(seqs)
    z[b, 0] = 0.0
    y[b, 0] = 0.0   # q - y == 0 exactly: the sub-gradient is 0, not -y/2
    edits[b] = ("zero", 0.0, 0)
    return Family(z, y, f.eta0, f.flag), edits, f


# the range forms (the pipelines' FTRL launches): (d, lanes)
RANGE_SHAPES = [(64, 8), (64, 16), (32, 8), (16, 8)]
RANGE_B, RANGE_T = 37, 100
RANGE_FAMILIES = ("gt_like", "straddle", "always")
RANGE_UNCLEAN = (12, RANGE_B - 1)


def range_case(name, d):
    """Family `name` with two sequences the closed form cannot certify: a row outside the ball
    in sequence 12, a label of 0.5 in the last sequence (the last wave-group)."""
    f = make(name, RANGE_B, RANGE_T, d, 900 + d)
    z, y = f.z.copy(), f.y.copy()
    z[12, RANGE_T // 2] *= 1.7
    y[RANGE_B - 1, 40] = 0.5
    return Family(z, y, f.eta0, f.flag)
