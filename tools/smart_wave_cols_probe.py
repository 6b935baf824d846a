"""Timing probe of the one-wave-per-sequence SMART sweeps (ocx_smart_wave_cols.hip): what M
thresholds, or K (horizon, threshold) pairs, cost in the bit-exact layout with flags 0 (the
reference's prefix re-scan) through every forced wave group and through the dispatcher, next
to two baselines that are both existing code and never the new kernel:

  loop   M calls of simulate_smart() (ocx_smart_wave_kernel); for a curve, K calls on K
         resident batches that hold the first t_k rows of the same data;
  lanes  the lane-group sweep, held by OCX_SMART_KERNEL=lanes (read at every call).

One JSON line per case, appended to profiles/smart_wave_cols_ab.jsonl (or --out).

  (t) thresholds on generate_gT batches 2 048 x 1e3 x {5, 16, 32, 64} and 32 768 x 1e3 x 5, M in
      {2, 4, 7}: sqrt(2T) and fractions of it (tools/thresholds_probe.py's), so the switches
      are spread over the horizon;
  (c) curves on 2 048 x 1e3 x 5 (one lane per sequence, 1 x 6), horizons 100 … 1000,
      thresholds scale * sqrt(2 t_k): scale 1 is never reached on these rows (every step of
      every column re-scans), 0.05 spreads the switches;
  (m) comparison_curves with g_emp on 2 048 x 1e3 x 5: the public call against itself on the
      lane-group kernel;
  (r) drivers.case_regrets' SMART and EMP at its own case sizes: the two simulate_smart
      launches against one two-column simulate_smart_thresholds call;
  (d) drivers.fast_driver_main() end to end, case_regrets as it stands against the two-launch
      form (wall clock, the sides alternating).

One process; device events on the stream around every repetition; 20 repetitions after 2
warm-up rounds; the sides of a comparison alternate repetition by repetition; median and
min-max.  --small runs toy sizes (a rehearsal of the script, not a measurement)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_convex_optimization_amd import drivers, engine  # noqa: E402

SQ2 = math.sqrt(2)
FRACTIONS = [1.0, 0.02, 0.05, 0.1, 0.2, 0.01, 0.5]   # tools/thresholds_probe.py
WAVE_GROUPS = (1, 2, 4, 8)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(sides, reps, warm=2, clock=timed):
    """{name: [ms] * reps}, the sides taking turns."""
    for _ in range(warm):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            ms[k].append(clock(fn))
    return ms


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
            "stdev_ms": statistics.pstdev(v), "reps": len(v)}


def held_on_lanes(fn):
    def run():
        os.environ["OCX_SMART_KERNEL"] = "lanes"
        try:
            return fn()
        finally:
            os.environ.pop("OCX_SMART_KERNEL", None)
    return run


def record(rec, ms, res, ref_reg, ref_sw):
    """Every side beside the two baselines: ratios of medians, whether the median lies outside
    each baseline's min-max, and the bits against the loop's."""
    rec["loop"], rec["lanes"] = stats(ms["loop"]), stats(ms["lanes"])
    for name in ms:
        s = stats(ms[name])
        if name not in ("loop", "lanes"):
            rec[name] = s
        rec[name].update(
            ratio_to_loop=s["median_ms"] / rec["loop"]["median_ms"],
            ratio_to_lanes=s["median_ms"] / rec["lanes"]["median_ms"],
            faster_than_both_outside_spread=bool(s["max_ms"] < rec["loop"]["min_ms"] and
                                                 s["max_ms"] < rec["lanes"]["min_ms"]))
        if name in res:
            rec[name].update(
                switch_steps_equal=bool(torch.equal(res[name]["switch_step"], ref_sw)),
                regrets_equal=bool(torch.equal(res[name]["regret"], ref_reg)))


def thresholds_case(out, B, T, d, reps, Ms):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=1).generate_gT(base_seed=0)
    assert db.exact
    for M in Ms:
        ths = [f * math.sqrt(2 * T) for f in FRACTIONS[:M]]
        sws = [torch.zeros(B, dtype=torch.int64, device=db.device) for _ in ths]
        regs = [None] * M
        res = {}

        def loop():
            for m, th in enumerate(ths):
                regs[m] = db.simulate_smart(th, SQ2, switch_step=sws[m], closed_prefix=False,
                                            closed_comparator=False)[:B].clone()

        def sweep(name, **kw):
            return lambda: res.__setitem__(name, db.simulate_smart_thresholds(ths, SQ2, **kw))

        sides = {"loop": loop, "lanes": held_on_lanes(sweep("lanes"))}
        for g in WAVE_GROUPS:
            sides[f"wave{g}"] = sweep(f"wave{g}", _wave=g)
        sides["auto"] = sweep("auto")
        ms = alternate(sides, reps)
        torch.cuda.synchronize()
        ref_sw, ref_reg = torch.stack(sws, dim=1), torch.stack(regs, dim=1)
        rec = {"case": "t", "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
               "M": M, "thresholds": ths,
               "mean_switch_step_per_column": ref_sw.double().mean(dim=0).cpu().tolist(),
               "never_switched_per_column": (ref_sw < 0).sum(dim=0).cpu().tolist()}
        record(rec, ms, res, ref_reg, ref_sw)
        out(rec)
    del db


def truncated(db, B, d, horizons, lanes):
    zr, yr = db.rows_of(torch.arange(B, device=db.device))
    cut = []
    for t in horizons:
        c = engine.DeviceBatch(B, t, d, lanes_per_seq=lanes).pack(zr[:, :t], yr[:, :t])
        assert (c.L.P, c.L.C, c.L.chain) == (db.L.P, db.L.C, db.L.chain)
        cut.append(c)
    torch.cuda.synchronize()
    del zr, yr
    for c in cut:
        c._keep = None
    torch.cuda.empty_cache()
    return cut


def curve_case(out, B, T, d, lanes, reps, horizons, scale):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes).generate_gT(base_seed=0)
    assert db.exact
    ths = [scale * math.sqrt(2 * t) for t in horizons]
    cut = truncated(db, B, d, horizons, lanes)
    sws = [torch.zeros(B, dtype=torch.int64, device=db.device) for _ in horizons]
    res = {}

    def loop():
        for c, th, sw in zip(cut, ths, sws):
            c.simulate_smart(th, SQ2, switch_step=sw, closed_prefix=False,
                             closed_comparator=False)

    def curve(name, **kw):
        return lambda: res.__setitem__(name, db.simulate_smart_curve(horizons, ths, SQ2, **kw))

    sides = {"loop": loop, "lanes": held_on_lanes(curve("lanes"))}
    for g in WAVE_GROUPS:
        sides[f"wave{g}"] = curve(f"wave{g}", _wave=g)
    sides["auto"] = curve("auto")
    ms = alternate(sides, reps)
    torch.cuda.synchronize()
    ref_sw = torch.stack(sws, dim=1)
    ref_reg = torch.stack([c.regret[:B] for c in cut], dim=1)
    rec = {"case": "c", "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
           "K": len(horizons), "horizons": list(horizons), "thresholds": ths, "scale": scale,
           "mean_switch_step_per_column": ref_sw.double().mean(dim=0).cpu().tolist(),
           "never_switched_per_column": (ref_sw < 0).sum(dim=0).cpu().tolist()}
    record(rec, ms, res, ref_reg, ref_sw)
    out(rec)
    del db, cut


def comparison_case(out, B, T, d, reps, horizons):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=1).generate_gT(base_seed=0)
    g_emp = [0.3 * math.sqrt(2 * t) for t in horizons]
    res = {}
    sides = {"lanes": held_on_lanes(
                 lambda: res.__setitem__("lanes", db.comparison_curves(horizons, g_emp))),
             "auto": lambda: res.__setitem__("auto", db.comparison_curves(horizons, g_emp))}
    ms = alternate(sides, reps)
    torch.cuda.synchronize()
    lanes, auto = stats(ms["lanes"]), stats(ms["auto"])
    out({"case": "m", "B": B, "T": T, "d": d, "K": len(horizons), "g_emp": g_emp,
         "lanes": lanes,
         "auto": dict(auto, ratio_to_lanes=auto["median_ms"] / lanes["median_ms"],
                      faster_outside_spread=bool(auto["max_ms"] < lanes["min_ms"]),
                      bits_equal=all(bool(torch.equal(res["auto"][k], res["lanes"][k]))
                                     for k in res["auto"]))})
    del db


def case_regrets_case(out, title, T, runs, replicates, g_emp_T, reps):
    family, stream0 = drivers.CASE_FAMILIES[title]
    B = runs * replicates
    db = engine.DeviceBatch(B, T, 5, lanes_per_seq=1)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    db.generate_family(family, 2025 * (run_idx + 1), stream0 + rep_idx, p=0.10, block_len=20)
    ths = [math.sqrt(2 * T), float(g_emp_T)]
    res = {}

    def two():
        res["two"] = [db.simulate_smart(th, SQ2).clone() for th in ths]

    sides = {"two_launches": two,
             "one_call": lambda: res.__setitem__("one", db.simulate_smart_thresholds(ths, SQ2))}
    ms = alternate(sides, reps)
    torch.cuda.synchronize()
    two_s, one_s = stats(ms["two_launches"]), stats(ms["one_call"])
    out({"case": "r", "title": title, "B": B, "T": T, "thresholds": ths,
         "two_launches": two_s,
         "one_call": dict(one_s, ratio=one_s["median_ms"] / two_s["median_ms"],
                          faster_outside_spread=bool(one_s["max_ms"] < two_s["min_ms"]),
                          bits_equal=all(bool(torch.equal(res["one"]["regret"][:, m],
                                                          res["two"][m][:B]))
                                         for m in range(2)))})
    del db


def two_launch_case_regrets(title, T, g_emp_T, *, runs, replicates, base_seed=0, d=5, p=0.10,
                            block_len=20, lanes_per_seq=1, device=0):
    """drivers.case_regrets with SMART and EMP from two simulate_smart launches."""
    family, stream0 = drivers.CASE_FAMILIES[title]
    B = runs * replicates
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes_per_seq, device=device)
    run_idx = np.repeat(np.arange(runs), replicates)
    rep_idx = np.tile(np.arange(replicates), runs)
    db.generate_family(family, base_seed + 2025 * (run_idx + 1), stream0 + rep_idx, p=p,
                       block_len=block_len)
    o = {"FTRL": db.simulate_alg(0, SQ2).clone(), "FTL": db.simulate_alg(1, SQ2).clone(),
         "SMART": db.simulate_smart(math.sqrt(2 * T), SQ2).clone(),
         "EMP": db.simulate_smart(float(g_emp_T), SQ2).clone()}
    return {k: v[:B].cpu().numpy().reshape(runs, replicates) for k, v in o.items()}


def driver_case(out, reps, T_grid):
    current = drivers.case_regrets
    res = {}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def run(name, impl):
        def go():
            drivers.case_regrets = impl
            try:
                res[name] = drivers.fast_driver_main(T_grid)
            finally:
                drivers.case_regrets = current
        return go

    sides = {"two_launches": run("two", two_launch_case_regrets),
             "as_committed": run("now", current)}
    ms = alternate(sides, reps, warm=1, clock=wall)
    two_s, now_s = stats(ms["two_launches"]), stats(ms["as_committed"])
    same = all(np.array_equal(a, b) for t in res["two"][1] for k in res["two"][1][t]
               for a, b in zip(res["two"][1][t][k], res["now"][1][t][k]))
    out({"case": "d", "T_grid": T_grid, "clock": "wall", "two_launches": two_s,
         "as_committed": dict(now_s, ratio=now_s["median_ms"] / two_s["median_ms"],
                              faster_outside_spread=bool(now_s["max_ms"] < two_s["min_ms"]),
                              stats_equal=bool(same))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "smart_wave_cols_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cases", default="tcmrd")
    ap.add_argument("--big", type=int, default=1, help="0: leave the 32 768 batch out")
    ap.add_argument("--dims", type=int, nargs="*", default=[5, 16, 32, 64],
                    help="d of the 2 048-sequence threshold cases")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def out(rec):
        rec["small"] = a.small
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    engine.release_buffers(0)
    k = 16 if a.small else 1
    T = 1000 // (4 if a.small else 1)
    horizons = [T * i // 10 for i in range(1, 11)]
    if "t" in a.cases:
        for d in a.dims:
            thresholds_case(out, 2048 // k, T, d, a.reps, (2, 4, 7))
            torch.cuda.empty_cache()
        if a.big:
            thresholds_case(out, 32768 // k, T, 5, a.reps, (2, 4, 7))
            torch.cuda.empty_cache()
    if "c" in a.cases:
        for d, lanes, scale in ((5, -1, 1.0), (5, -1, 0.05)):
            curve_case(out, 2048 // k, T, d, lanes, a.reps, horizons, scale)
            torch.cuda.empty_cache()
    if "m" in a.cases:
        comparison_case(out, 2048 // k, T, 5, a.reps, horizons)
        torch.cuda.empty_cache()
    if "r" in a.cases:
        Ts = [T // 10, T]
        g_emp = drivers.empirical_worst_case_thresholds(np.asarray(Ts), runs=1000 // k,
                                                        base_seed=0)
        for title in ("Random i.i.d. (separable)", "Massart noise 10%", "Label flips"):
            for Tn in Ts:
                case_regrets_case(out, title, Tn, drivers.RUNS_BY_TITLE[title],
                                  drivers.REPLICATES_BY_TITLE[title], g_emp[Tn], a.reps)
    if "d" in a.cases:
        driver_case(out, 3 if a.small else 5, horizons)


if __name__ == "__main__":
    main()
