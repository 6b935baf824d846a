"""A/B timing of the float32 twin's column sweeps against the single calls.

    python tools/twin32_cols_probe.py > profiles/twin32_cols_ab.jsonl

Three legs, each interleaving its variants rep by rep in one process (torch events on the
batch's stream around the launches; wall clock for the driver), one JSON line per leg with
median / min / max / stdev per variant and a bit-equality check of the results:
  1. 2 048 x 1e3 x 5, i.i.d. family: one 4-column call (FTRL, FTL, SMART sqrt(2T), EMP 4.2)
     against the four DeviceBatch.simulate_twin32 calls; also the column call at forced groups.
  2. the same batch: twin32_comparison_curves(range(100, 1100, 100), g_emp) (40 columns) against
     the 40 single calls on ten truncated resident batches (built outside the timed region).
  3. drivers.driver_main() with case_regrets_twin32 on four single calls (as it was; swapped in
     for the measurement only) and on its one 4-column call.
"""
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_convex_optimization_amd import drivers, engine  # noqa: E402

SQ2 = math.sqrt(2)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "stdev_ms": statistics.pstdev(ms), "reps": len(ms)}


def ab(variants, reps, timer):
    """Interleaved: one rep of every variant per round, after one warm-up round."""
    for fn in variants.values():
        fn()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            ms[k].append(timer(fn))
    return {k: stats(v) for k, v in ms.items()}


def event_timer(torch, stream):
    def timer(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    return timer


def wall_timer(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def rows(db):
    """(z [B, T, d], y [B, T]) float64 device tensors of a one-lane resident batch."""
    L = db.L
    z = db.z[:L.z_elems].view(L.C // 2, L.G, L.T, 64, 2).permute(1, 3, 2, 0, 4)
    z = z.reshape(L.G * 64, L.T, L.C)[:L.B, :, :L.d].contiguous()
    y = db.y[:L.y_elems].view(L.G, L.T, 64).permute(0, 2, 1).reshape(L.G * 64, L.T)[:L.B]
    return z, y.contiguous()


def case_regrets_twin32_four(title, T, g_emp_T, *, runs, replicates, base_seed=0, d=5, p=0.10,
                             block_len=20, device=0):
    """drivers.case_regrets_twin32 as it was before the column call: four single launches."""
    family, stream0 = drivers.CASE_FAMILIES[title]
    B = runs * replicates
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=-1, device=device)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    db.generate_family(family, base_seed + 2025 * (run_idx + 1), stream0 + rep_idx, p=p,
                       block_len=block_len)
    out = {"FTRL": db.simulate_twin32(0, SQ2), "FTL": db.simulate_twin32(1, SQ2),
           "SMART": db.simulate_twin32(2, SQ2, math.sqrt(2 * T)),
           "EMP": db.simulate_twin32(2, SQ2, float(g_emp_T))}
    return {k: v[:B].cpu().numpy().reshape(runs, replicates) for k, v in out.items()}


def main():
    import torch
    legs = set(sys.argv[1:]) or {"1", "2", "3"}
    B, T, d = 2048, 1000, 5
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=-1)
    b = np.arange(B)
    db.generate_family("iid", 2025 * (b // 8 + 1), 13 + b % 8)
    timer = event_timer(torch, db.stream)
    g42 = 4.2

    if "1" in legs:
        hz, al = [T] * 4, [0, 1, 2, 2]
        th = [np.nan, np.nan, math.sqrt(2 * T), g42]

        def four():
            return [db.simulate_twin32(0, SQ2), db.simulate_twin32(1, SQ2),
                    db.simulate_twin32(2, SQ2, math.sqrt(2 * T)), db.simulate_twin32(2, SQ2, g42)]

        def cols(g=None):
            return db.simulate_twin32_cols(hz, al, th, SQ2, _group=g)

        want = torch.stack([r[:B] for r in four()], dim=1).cpu().numpy()
        out = cols()
        sw = out["switch_step"].cpu().numpy()
        rec = {"leg": 1, "B": B, "T": T, "d": d, "columns": ["FTRL", "FTL", "SMART sqrt(2T)", "EMP 4.2"],
               "results_equal": bool(np.array_equal(out["result"].cpu().numpy(), want)),
               "never_switched": [int((sw[:, k] < 0).sum()) for k in (2, 3)],
               "mean_switch_step": [float(sw[:, k][sw[:, k] >= 0].mean()) if (sw[:, k] >= 0).any()
                                    else -1.0 for k in (2, 3)]}
        rec.update(ab({"four_calls": four, "cols": cols, "cols_group1": lambda: cols(1),
                       "cols_group2": lambda: cols(2), "cols_group4": lambda: cols(4)}, 15, timer))
        rec["ratio_cols_to_four_calls"] = rec["cols"]["median_ms"] / rec["four_calls"]["median_ms"]
        print(json.dumps(rec), flush=True)

    if "2" in legs:
        grid = list(range(100, 1100, 100))
        # a plausible g(t): the twin's empirical thresholds grow like sqrt(t)
        g_emp = [0.42 * math.sqrt(t) for t in grid]
        z, y = rows(db)
        cut = []
        for t in grid:
            c = engine.DeviceBatch(B, t, d, lanes_per_seq=-1, stream=db.stream)
            c.pack(z[:, :t].contiguous(), y[:, :t].contiguous())
            cut.append(c)

        def forty():
            return [[c.simulate_twin32(0, SQ2), c.simulate_twin32(1, SQ2),
                     c.simulate_twin32(2, SQ2, math.sqrt(2 * t)), c.simulate_twin32(2, SQ2, g)]
                    for c, t, g in zip(cut, grid, g_emp)]

        def curves():
            return db.twin32_comparison_curves(grid, g_emp, SQ2)

        want = forty()
        got = curves()
        eq = all(np.array_equal(got[k][:B, ti].cpu().numpy(), want[ti][i][:B].cpu().numpy())
                 for ti in range(len(grid)) for i, k in enumerate(drivers.ALGO_KEYS))
        rec = {"leg": 2, "B": B, "T": T, "d": d, "grid": grid, "g_emp": g_emp, "columns": 40,
               "results_equal": bool(eq)}
        rec.update(ab({"forty_calls": forty, "curves": curves}, 7, timer))
        rec["ratio_curves_to_forty_calls"] = (rec["curves"]["median_ms"] /
                                              rec["forty_calls"]["median_ms"])
        print(json.dumps(rec), flush=True)

    if "3" in legs:
        cols = drivers.case_regrets_twin32  # one 4-column call

        def run(fn):
            drivers.case_regrets_twin32 = fn
            try:
                return drivers.driver_main()
            finally:
                drivers.case_regrets_twin32 = cols

        a, c = run(case_regrets_twin32_four), run(cols)
        eq = all(np.array_equal(a[1][t][k][i], c[1][t][k][i])
                 for t in a[1] for k in a[1][t] for i in (0, 1))
        rec = {"leg": 3, "what": "drivers.driver_main(), wall clock", "stats_equal": bool(eq)}
        rec.update(ab({"four_calls": lambda: run(case_regrets_twin32_four),
                       "cols": lambda: run(cols)}, 5, wall_timer))
        rec["ratio_cols_to_four_calls"] = rec["cols"]["median_ms"] / rec["four_calls"]["median_ms"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
