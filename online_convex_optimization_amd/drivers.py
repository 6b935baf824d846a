"""Batched, device-resident versions of the reference's experiment sweeps
(fast_driver.py and exact_ftl_driver.py).

``evaluate_stream_with_stats`` (fast_driver.py:71-127) calls simulate_alg / SMART
once per (run, T, replicate) on host-built sequences.  Here every (run, replicate)
sequence of one T is generated on the GPU in a single batch (its ``sequence_generation``
family, bit-identical to the NumPy streams), the four algorithms run as four kernel
launches over that batch, and only the 4·runs·replicates regrets come back.  The
averaging then uses the same NumPy calls as the reference (fast_driver.py:113-125), so
the statistics are identical, not merely close.

``fast_driver_main`` is fast_driver.py:201-220 without the plotting: the g(T) sweep
(empirical_worst_case_thresholds) followed by the four cases.  ``driver_main`` is the
same for driver.py:204-226, which runs the float32 twin (algorithms.py).
"""
from __future__ import annotations

import math
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import engine
from .fast_algorithms import empirical_worst_case_thresholds
from .sequence_generation import REPLICATES_BY_TITLE, RUNS_BY_TITLE

ALGO_KEYS = ("FTRL", "FTL", "SMART", "EMP")
CI_Z = 1.96
SQRT2 = math.sqrt(2)

# CASES title → (device family, stream-id base of the replicate streams, d)
CASE_FAMILIES = {
    "Random i.i.d. (separable)": ("iid", 13),
    "Massart noise 10%": ("massart", 23),
    "Label flips": ("flip", 0),
    "Switching leaders": ("switching", 0),
}

Stats = Dict[str, Tuple[np.ndarray, np.ndarray]]


def _sem(x: np.ndarray) -> float:
    """fast_driver.py:59-63."""
    n = x.size
    if n <= 1:
        return 0.0
    return float(np.std(x, ddof=1) / math.sqrt(n))


def case_regrets(title: str, T: int, g_emp_T: float, *, runs: int, replicates: int,
                 base_seed: int = 0, d: int = 5, p: float = 0.10, block_len: int = 20,
                 lanes_per_seq: int = 1, device: int = 0) -> Dict[str, np.ndarray]:
    """Regrets [runs, replicates] of FTRL, FTL, SMART(sqrt 2T), SMART(g_emp) for one case
    and one T — fast_driver.py:86-111 for every (run, rep) at once, on device."""
    family, stream0 = CASE_FAMILIES[title]
    B = runs * replicates
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes_per_seq, device=device)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    run_seeds = base_seed + 2025 * (run_idx + 1)  # fast_driver.py:88
    db.generate_family(family, run_seeds, stream0 + rep_idx, p=p, block_len=block_len)
    out = {}
    out["FTRL"] = db.simulate_alg(0, SQRT2).clone()
    out["FTL"] = db.simulate_alg(1, SQRT2).clone()
    # SMART and EMP share their FTL leg and every prefix re-scan up to the later switch: one
    # two-column sweep, the bits of two simulate_smart launches
    both = db.simulate_smart_thresholds([math.sqrt(2 * T), float(g_emp_T)], SQRT2)["regret"]
    out["SMART"], out["EMP"] = both[:, 0], both[:, 1]
    return {k: v[:B].cpu().numpy().reshape(runs, replicates) for k, v in out.items()}


def case_threshold_regrets(title: str, T: int, thresholds, *, runs: int, replicates: int,
                           base_seed: int = 0, d: int = 5, p: float = 0.10, block_len: int = 20,
                           lanes_per_seq: int = 1, device: int = 0
                           ) -> Tuple[np.ndarray, np.ndarray]:
    """SMART's regret against its switch threshold for one case and one T: (regrets
    [runs, replicates, M], switch_steps [runs, replicates, M], -1 = never switched) for the
    M values of ``thresholds``, on the batch case_regrets generates (the same sequences),
    through one threshold sweep (DeviceBatch.simulate_smart_thresholds) instead of one SMART
    run per threshold.  ``sqrt(2T)`` and the empirical g(T) are case_regrets' SMART and EMP;
    ``thresh = +inf`` never switches and is its FTL, with the same adds and the same
    comparator."""
    family, stream0 = CASE_FAMILIES[title]
    B = runs * replicates
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes_per_seq, device=device)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    run_seeds = base_seed + 2025 * (run_idx + 1)  # fast_driver.py:88
    db.generate_family(family, run_seeds, stream0 + rep_idx, p=p, block_len=block_len)
    out = db.simulate_smart_thresholds(thresholds, SQRT2)
    M = int(out["regret"].shape[1])
    return (out["regret"].cpu().numpy().reshape(runs, replicates, M),
            out["switch_step"].cpu().numpy().reshape(runs, replicates, M))


def case_threshold_regret_grid(title: str, checkpoints, thresholds, *, runs: int,
                               replicates: int, base_seed: int = 0, d: int = 5, p: float = 0.10,
                               block_len: int = 20, lanes_per_seq: int = 1, device: int = 0
                               ) -> Tuple[np.ndarray, np.ndarray]:
    """SMART's regret against its switch threshold AND the horizon for one case: (regrets
    [runs, replicates, M, K], switch_steps [runs, replicates, M, K], -1 = not switched before
    t_k) for the M values of ``thresholds`` at the K horizons of ``checkpoints`` (strictly
    increasing), on the batch case_threshold_regrets generates at T = t_K (the same
    sequences), through one regret grid (DeviceBatch.simulate_smart_grid): every threshold
    runs once, to t_K, and is read at every checkpoint on the way.

    What the columns are depends on the family.  For the deterministic families (label flips,
    switching leaders) the prefix of the long sequence IS the reference's sequence at each T,
    so [..., k] holds case_threshold_regrets(title, t_k, thresholds), bit for bit.  For the
    random families (i.i.d., Massart) the reference draws a fresh sequence per T
    (sequence_generation.py:61-62: the generator is seeded with T), so the grid is the anytime
    regret on the longest horizon's rows — a different sample of the same distribution, not
    the reference's per-T numbers."""
    family, stream0 = CASE_FAMILIES[title]
    grid = np.asarray(checkpoints)
    ck = engine._checkpoints(grid, int(grid.max()) if grid.size else 0)  # ValueError if bad
    B, K = runs * replicates, int(ck.size)
    M = int(engine._thresholds(thresholds, B).shape[1])
    if B == 0 or K == 0 or M == 0:
        return (np.zeros((runs, replicates, M, K)),
                np.full((runs, replicates, M, K), -1, dtype=np.int64))
    db = engine.DeviceBatch(B, int(ck[-1]), d, lanes_per_seq=lanes_per_seq, device=device)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    run_seeds = base_seed + 2025 * (run_idx + 1)  # fast_driver.py:88
    db.generate_family(family, run_seeds, stream0 + rep_idx, p=p, block_len=block_len)
    out = db.simulate_smart_grid(ck, thresholds, SQRT2)
    return (out["regret"][:B].cpu().numpy().reshape(runs, replicates, M, K),
            out["switch_step"][:B].cpu().numpy().reshape(runs, replicates, M, K))


def evaluate_stream_with_stats(title: str, T_grid: Sequence[int], g_emp: Mapping[int, float], *,
                               runs: int = 1, replicates: int = 1, base_seed: int = 0,
                               lanes_per_seq: int = 1, device: int = 0) -> Stats:
    """fast_driver.py:71-127 for the CASES entry ``title``: mean regret and 95 % CI per T."""
    by_T = {k: [[] for _ in range(len(T_grid))] for k in ALGO_KEYS}
    per_T = [case_regrets(title, int(T), g_emp[int(T)], runs=runs, replicates=replicates,
                          base_seed=base_seed, lanes_per_seq=lanes_per_seq, device=device)
             for T in T_grid]
    for run in range(runs):
        for ti in range(len(T_grid)):
            for k in ALGO_KEYS:
                by_T[k][ti].append(float(np.mean(list(per_T[ti][k][run]))))
    stats: Stats = {}
    for k in ALGO_KEYS:
        means, cis = [], []
        for vals in by_T[k]:
            arr = np.asarray(vals, dtype=float)
            mu = float(np.mean(arr)) if arr.size else 0.0
            ci = CI_Z * _sem(arr) if arr.size > 1 else 0.0
            means.append(mu)
            cis.append(ci)
        stats[k] = (np.array(means, dtype=float), np.array(cis, dtype=float))
    return stats


def fast_driver_main(T_grid: Optional[Sequence[int]] = None, *, g_runs: int = 1000,
                     base_seed: int = 0, runs_by_title: Optional[Mapping[str, int]] = None,
                     replicates_by_title: Optional[Mapping[str, int]] = None,
                     device: int = 0) -> Tuple[Dict[int, float], Dict[str, Stats]]:
    """fast_driver.py:201-220 minus the figures: (g_emp, stats_by_case)."""
    T_grid = list(range(100, 1100, 100)) if T_grid is None else [int(t) for t in T_grid]
    runs_by_title = RUNS_BY_TITLE if runs_by_title is None else runs_by_title
    replicates_by_title = REPLICATES_BY_TITLE if replicates_by_title is None else replicates_by_title
    g_emp = empirical_worst_case_thresholds(np.asarray(T_grid), runs=g_runs, base_seed=base_seed)
    stats = {}
    for title in CASE_FAMILIES:
        stats[title] = evaluate_stream_with_stats(
            title, T_grid, g_emp, runs=runs_by_title.get(title, 1),
            replicates=replicates_by_title.get(title, 1), base_seed=base_seed, device=device)
    return g_emp, stats


# ---------------------------------------------------------------------------
# driver.py: the same sweep on the float32 twin (algorithms.py)
# ---------------------------------------------------------------------------

def case_regrets_twin32(title: str, T: int, g_emp_T: float, *, runs: int, replicates: int,
                        base_seed: int = 0, d: int = 5, p: float = 0.10, block_len: int = 20,
                        device: int = 0) -> Dict[str, np.ndarray]:
    """driver.py:86-111 for every (run, rep) of one case and T at once: the four twin
    algorithms (algorithms.py) on the device-generated family, float32 regrets
    [runs, replicates]."""
    family, stream0 = CASE_FAMILIES[title]
    B = runs * replicates
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=-1, device=device)  # one lane per sequence
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    db.generate_family(family, base_seed + 2025 * (run_idx + 1), stream0 + rep_idx, p=p,
                       block_len=block_len)
    # The four lines share one staging of the rows and one prefix re-scan per step: one
    # 4-column call, the bits of four simulate_twin32 launches
    th = [math.sqrt(2 * T), float(g_emp_T)]  # driver.py:95 float(g_emp[T])
    try:
        res = db.simulate_twin32_cols([T] * 4, [0, 1, 2, 2], [np.nan, np.nan, *th],
                                      SQRT2)["result"][:B].cpu().numpy()
    except NotImplementedError:  # T rows do not fit the LDS: the single calls' lane kernel
        out = {"FTRL": db.simulate_twin32(0, SQRT2), "FTL": db.simulate_twin32(1, SQRT2),
               "SMART": db.simulate_twin32(2, SQRT2, th[0]),
               "EMP": db.simulate_twin32(2, SQRT2, th[1])}
        return {k: v[:B].cpu().numpy().reshape(runs, replicates) for k, v in out.items()}
    return {k: res[:, i].reshape(runs, replicates) for i, k in enumerate(ALGO_KEYS)}


def driver_case_regret_curves(title: str, T_grid: Sequence[int], g_emp: Mapping[int, float], *,
                              runs: int, replicates: int, base_seed: int = 0, d: int = 5,
                              p: float = 0.10, block_len: int = 20, device: int = 0
                              ) -> Dict[str, np.ndarray]:
    """The four lines of case_regrets_twin32 against the horizon, from ONE batch: the case's
    sequences are generated once at horizon max(T_grid) and the float32 twin is read at every
    T of ``T_grid`` (strictly increasing) by one column call
    (DeviceBatch.twin32_comparison_curves: 4K columns, one staging of the rows and one prefix
    re-scan per step for a group of them).  ``g_emp`` maps T to the empirical threshold, as
    in driver_evaluate_stream_with_stats.  Returns {"FTRL", "FTL", "SMART", "EMP"}, float32
    [runs * replicates, K] each; column k is the twin's regret on the first T_k rows of that
    batch.

    What the columns are depends on the family.  For the deterministic families (label flips,
    switching leaders) the prefix of the long sequence IS the reference's sequence at each T,
    so column k holds the reference's numbers: case_regrets_twin32(title, T_k, g_emp[T_k]),
    bit for bit.  For the random families (i.i.d., Massart) the reference draws a fresh
    sequence per T (sequence_generation.py:61-62: the generator is seeded with T), so the
    curve is the anytime regret on the longest horizon's rows — a different sample of the
    same distribution, not the reference's per-T numbers.
    driver_evaluate_stream_with_stats therefore keeps one batch per T."""
    family, stream0 = CASE_FAMILIES[title]
    grid = np.asarray(T_grid)
    ck = engine._checkpoints(grid, int(grid.max()) if grid.size else 0)  # ValueError if bad
    B, K = runs * replicates, int(ck.size)
    if B == 0 or K == 0:
        return {k: np.zeros((B, K), dtype=np.float32) for k in ALGO_KEYS}
    g = np.array([float(g_emp[int(T)]) for T in ck])  # driver.py:95 float(g_emp[T])
    db = engine.DeviceBatch(B, int(ck[-1]), d, lanes_per_seq=-1, device=device)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    db.generate_family(family, base_seed + 2025 * (run_idx + 1), stream0 + rep_idx, p=p,
                       block_len=block_len)
    out = db.twin32_comparison_curves(ck, g, SQRT2)
    return {k: out[k][:B].cpu().numpy() for k in ALGO_KEYS}


def driver_evaluate_stream_with_stats(title: str, T_grid: Sequence[int],
                                      g_emp: Mapping[int, float], *, runs: int = 1,
                                      replicates: int = 1, base_seed: int = 0,
                                      device: int = 0) -> Stats:
    """driver.py:70-136 for the CASES entry ``title`` (float32 twin): mean regret and 95 % CI
    per T, the replicate means taken over the twin's np.float32 values as driver.py does."""
    by_T = {k: [[] for _ in range(len(T_grid))] for k in ALGO_KEYS}
    per_T = [case_regrets_twin32(title, int(T), g_emp[int(T)], runs=runs, replicates=replicates,
                                 base_seed=base_seed, device=device) for T in T_grid]
    for run in range(runs):
        for ti in range(len(T_grid)):
            for k in ALGO_KEYS:
                by_T[k][ti].append(float(np.mean(list(per_T[ti][k][run]))))
    stats: Stats = {}
    for k in ALGO_KEYS:
        means, cis = [], []
        for vals in by_T[k]:
            arr = np.asarray(vals, dtype=float)
            means.append(float(np.mean(arr)) if arr.size else 0.0)
            cis.append(CI_Z * _sem(arr) if arr.size > 1 else 0.0)
        stats[k] = (np.array(means, dtype=float), np.array(cis, dtype=float))
    return stats


def driver_main(T_grid: Optional[Sequence[int]] = None, *, g_runs: int = 1000,
                base_seed: int = 0, runs_by_title: Optional[Mapping[str, int]] = None,
                replicates_by_title: Optional[Mapping[str, int]] = None,
                device: int = 0):
    """driver.py:204-226 minus the figures (float32 twin): (g_emp, stats_by_case)."""
    from . import algorithms
    T_grid = list(range(100, 1100, 100)) if T_grid is None else [int(t) for t in T_grid]
    runs_by_title = RUNS_BY_TITLE if runs_by_title is None else runs_by_title
    replicates_by_title = REPLICATES_BY_TITLE if replicates_by_title is None else replicates_by_title
    g_emp = algorithms.empirical_worst_case_thresholds(np.asarray(T_grid), runs=g_runs,
                                                       base_seed=base_seed)
    stats = {}
    for title in CASE_FAMILIES:
        stats[title] = driver_evaluate_stream_with_stats(
            title, T_grid, g_emp, runs=runs_by_title.get(title, 1),
            replicates=replicates_by_title.get(title, 1), base_seed=base_seed, device=device)
    return g_emp, stats


# ---------------------------------------------------------------------------
# exact_ftl_driver.py: FTRL against the exact comparator, exact FTL replay
# ---------------------------------------------------------------------------
EXACT_ALGOS = ("FTRL", "FTL (exact)")


def exact_case_regrets(title: str, T: int, *, runs: int, replicates: int, base_seed: int = 0,
                       d: int = 5, p: float = 0.10, block_len: int = 20, lanes_per_seq: int = 1,
                       device: int = 0, norm: str = "l2") -> Dict[str, np.ndarray]:
    """exact_ftl_driver.py:157-186 for every (run, rep) of one case and T on device:
    exact FTL prefix actions over the ``norm`` ball (ExperimentConfig.norm, :46; closed
    form in its regime, else the general solver) replayed → "FTL (exact)" regret; FTRL
    (eta0 = sqrt 2) against actions[T] → "FTRL" regret."""
    import torch
    family, stream0 = CASE_FAMILIES[title]
    B = runs * replicates
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes_per_seq, device=device)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    db.generate_family(family, base_seed + 2025 * (run_idx + 1), stream0 + rep_idx, p=p,
                       block_len=block_len)
    return _exact_pair(db, B, d, torch, norm)


def _exact_pair(db, B, d, torch, norm: str = "l2") -> Dict[str, np.ndarray]:
    """Both regrets of exact_ftl_driver.py:169-184 in one read of the batch
    (ocx_dev_ftrl_vs_exact): FTRL and exact FTL against the exact comparator actions[T];
    sequences outside the closed form's regime take the general solver."""
    db.ftrl_vs_exact_general(SQRT2, norm=norm)
    ftrl = db.cum - db.comp
    ftl = db.cum_exact - db.comp
    return {"FTRL": ftrl[:B].cpu().numpy(), "FTL (exact)": ftl[:B].cpu().numpy()}


def exact_case_regret_curves(title: str, T_grid: Sequence[int], *, runs: int, replicates: int,
                             base_seed: int = 0, d: int = 5, p: float = 0.10,
                             block_len: int = 20, lanes_per_seq: int = 1, device: int = 0,
                             norm: str = "l2") -> Dict[str, np.ndarray]:
    """Both regrets of exact_case_regrets against the horizon, from ONE batch: the case's
    sequences are generated once at horizon max(T_grid) and the curve
    (DeviceBatch.ftrl_vs_exact_curve_general) is read at every T of ``T_grid`` (strictly
    increasing) in one pass.  Returns {"FTRL", "FTL (exact)"}, each [runs * replicates, K];
    column k is the regret on the first T_k rows of that batch.

    What the columns are depends on the family.  For the deterministic families (label flips,
    switching leaders) the prefix of the long sequence IS the reference's sequence at each T,
    so column k holds the reference's numbers: exact_case_regrets(title, T_k), bit for bit.
    For the random families (i.i.d., Massart) the reference draws a fresh sequence per T
    (sequence_generation.py:61-62: the generator is seeded with T), so the curve is the
    anytime regret on the longest horizon's rows — a different sample of the same
    distribution, not the reference's per-T numbers.  exact_evaluate_stream_with_stats
    therefore keeps one batch per T."""
    family, stream0 = CASE_FAMILIES[title]
    grid = np.asarray(T_grid)
    ck = engine._checkpoints(grid, int(grid.max()) if grid.size else 0)  # ValueError if bad
    B, K = runs * replicates, int(ck.size)
    if B == 0 or K == 0:
        return {k: np.zeros((B, K)) for k in EXACT_ALGOS}
    db = engine.DeviceBatch(B, int(ck[-1]), d, lanes_per_seq=lanes_per_seq, device=device)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    db.generate_family(family, base_seed + 2025 * (run_idx + 1), stream0 + rep_idx, p=p,
                       block_len=block_len)
    out = db.ftrl_vs_exact_curve_general(ck, SQRT2, norm=norm)
    return {"FTRL": out["ftrl"][:B].cpu().numpy(), "FTL (exact)": out["exact"][:B].cpu().numpy()}


def exact_case_regret_grid(title: str, T_grid: Sequence[int], etas, *, runs: int,
                           replicates: int, base_seed: int = 0, d: int = 5, p: float = 0.10,
                           block_len: int = 20, lanes_per_seq: int = 1, device: int = 0,
                           norm: str = "l2") -> Dict[str, np.ndarray]:
    """exact_case_regret_curves for every FTRL step size of ``etas`` (a one-dimensional list of
    reals), from ONE batch generated at horizon max(T_grid) and one grid call
    (DeviceBatch.ftrl_vs_exact_curve_etas_general): {"FTRL": [runs * replicates, M, K],
    "FTL (exact)": [runs * replicates, K]}.  "FTRL"[:, m, :] is exact_case_regret_curves' FTRL
    line with eta0 = etas[m] in place of sqrt 2; the exact-FTL line does not depend on the step
    size.

    What the columns are depends on the family, as for exact_case_regret_curves.  For the
    deterministic families (label flips, switching leaders) the prefix of the long sequence IS
    the reference's sequence at each T, so column k holds the reference's numbers at T_k.  For
    the random families (i.i.d., Massart) the reference draws a fresh sequence per T
    (sequence_generation.py:61-62: the generator is seeded with T), so the grid is the anytime
    regret on the longest horizon's rows — a different sample of the same distribution, not
    the reference's per-T numbers."""
    family, stream0 = CASE_FAMILIES[title]
    grid = np.asarray(T_grid)
    ck = engine._checkpoints(grid, int(grid.max()) if grid.size else 0)  # ValueError if bad
    et = engine._etas(etas)
    B, K, M = runs * replicates, int(ck.size), int(et.size)
    if B == 0 or K == 0 or M == 0:
        return {"FTRL": np.zeros((B, M, K)), "FTL (exact)": np.zeros((B, K))}
    db = engine.DeviceBatch(B, int(ck[-1]), d, lanes_per_seq=lanes_per_seq, device=device)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    db.generate_family(family, base_seed + 2025 * (run_idx + 1), stream0 + rep_idx, p=p,
                       block_len=block_len)
    out = db.ftrl_vs_exact_curve_etas_general(ck, et, norm=norm)
    return {"FTRL": out["ftrl"][:B].cpu().numpy(), "FTL (exact)": out["exact"][:B].cpu().numpy()}


def exact_evaluate_stream_with_stats(title: str, T_grid: Sequence[int], *, runs: int,
                                     replicates: int, base_seed: int = 0, device: int = 0,
                                     norm: str = "l2") -> Stats:
    """exact_ftl_driver.py:120-206 for the CASES entry ``title``."""
    by_T = {k: [[] for _ in range(len(T_grid))] for k in EXACT_ALGOS}
    per_T = []
    for T in T_grid:
        r = exact_case_regrets(title, int(T), runs=runs, replicates=replicates,
                               base_seed=base_seed, device=device, norm=norm)
        per_T.append({k: v.reshape(runs, replicates) for k, v in r.items()})
    for run in range(runs):
        for ti in range(len(T_grid)):
            for k in EXACT_ALGOS:
                by_T[k][ti].append(float(np.mean(list(per_T[ti][k][run]))))
    stats: Stats = {}
    for k in EXACT_ALGOS:
        means, cis = [], []
        for vals in by_T[k]:
            arr = np.asarray(vals, dtype=float)
            means.append(float(np.mean(arr)) if arr.size else 0.0)
            cis.append(CI_Z * _sem(arr) if arr.size > 1 else 0.0)
        stats[k] = (np.array(means, dtype=float), np.array(cis, dtype=float))
    return stats


def exact_empirical_worst_case_thresholds(T_grid: Sequence[int], *, runs: int = 200,
                                          base_seed: int = 0, d: int = 5, device: int = 0,
                                          norm: str = "l2") -> Dict[int, float]:
    """exact_ftl_driver.py:64-117: max over runs of FTRL's regret against the exact
    comparator, on the g(T) adversary regenerated on device."""
    import torch
    g = {}
    for T in T_grid:
        T = int(T)
        db = engine.DeviceBatch(runs, T, d, lanes_per_seq=1, device=device)
        db.generate_gT(base_seed, 0)
        r = _exact_pair(db, runs, d, torch, norm)["FTRL"]
        g[T] = engine.max_regret(r)
    return g


def exact_ftl_driver_main(T_grid: Optional[Sequence[int]] = None, *, g_runs: int = 200,
                          base_seed: int = 0, device: int = 0, norm: str = "l2"):
    """exact_ftl_driver.py:268-293 minus the figures: (g_emp, stats_by_case); ``norm`` is
    ExperimentConfig.norm (:46)."""
    T_grid = list(range(100, 1100, 100)) if T_grid is None else [int(t) for t in T_grid]
    g = exact_empirical_worst_case_thresholds(T_grid, runs=g_runs, base_seed=base_seed,
                                              device=device, norm=norm)
    stats = {t: exact_evaluate_stream_with_stats(t, T_grid, runs=RUNS_BY_TITLE.get(t, 1),
                                                 replicates=REPLICATES_BY_TITLE.get(t, 1),
                                                 base_seed=base_seed, device=device, norm=norm)
             for t in CASE_FAMILIES}
    return g, stats
