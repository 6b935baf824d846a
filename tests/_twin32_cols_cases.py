"""Inputs of the twin column tests (test_twin32_cols_cpu.py, test_gpu_twin32_cols.py).

B = 70 crosses a 64-sequence tile; the horizons hit n = 1 (sgemv's one-row sdot rule), every
n mod 4 (sgemv's tail rows) and prefixes on both sides of the 128-element pairwise leaf; seven
columns leave a tail group at 2 and 4 columns per launch.  The CPU test asserts with the oracle
that these thresholds split the sequences at every middle horizon (some switched before t_k,
some only after it), so a kernel that ignores or misplaces a horizon cannot pass."""
import functools
import math

import numpy as np

F = np.float32
SQ2 = math.sqrt(2)
DIMS = (1, 5, 8, 16)
B, T = 70, 257
CK7 = [1, 37, 64, 102, 144, 199, 257]
TH7 = [-1, 2, 3, np.inf, 5, 6, 7]
MID = (1, 2, 4, 5)  # columns with a finite threshold and a horizon strictly inside (1, T)
INF_COL = 3


@functools.lru_cache(maxsize=None)
def case(d: int):
    """(z [B, T, d] float32, y [B, T] float32) of dimension d; shared, do not modify."""
    rng = np.random.default_rng(4100 + d)
    z = (rng.standard_normal((B, T, d)) * rng.choice([0.2, 0.5, 1.5], size=(B, 1, 1))).astype(F)
    y = np.where(rng.random((B, T)) < 0.5, -1.0, 1.0).astype(F)
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


@functools.lru_cache(maxsize=None)
def oracle_full_switch(d: int) -> np.ndarray:
    """[B, len(TH7)] int64: the oracle's switch step of the full run (all T rows) at every
    threshold of TH7, -1 = never.  A run truncated at t_k is the first t_k steps of this run,
    so column k has switched before t_k iff 0 <= step < t_k.  Computed once per d."""
    from oracle import oracle as O
    z, y = case(d)
    out = np.full((B, len(TH7)), -1, dtype=np.int64)
    for k, th in enumerate(TH7):
        for b in range(B):
            out[b, k] = O.t32_simulate_smart_full(z[b], y[b], float(th), SQ2)[3]
    out.setflags(write=False)
    return out


# the mixed list: FTRL, FTL and SMART at repeated horizons, K = 9 (more than one launch at
# every group size); NaN = no threshold (FTRL / FTL columns)
MIX_HZ = [0, 1, 37, 37, 37, 102, 102, 257, 257]
MIX_ALGO = ["FTRL", "SMART", "FTRL", "FTL", "SMART", "SMART", "FTL", "FTRL", "SMART"]
MIX_TH = [np.nan, 0.5, np.nan, np.nan, 2.0, np.inf, np.nan, np.nan, 6.0]
ALGO_CODE = {"FTRL": 0, "FTL": 1, "SMART": 2}
