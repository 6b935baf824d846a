"""Anytime-regret timing probe: what evaluating the closed-form regret at EVERY step costs next
to one curve pass, on resident generate_gT batches.  One JSON line per case, appended to
profiles/anytime_ab.jsonl (or --out).

  (a) 32 768 x 1e4 x 64 at 8 x 8 (the pipelined loop, HBM-bound);
  (b) 65 536 x 1e3 x 5 (the plain loop);
  (c) 4 900 x 1e5 x 64 (few waves, issue-bound: where the extra butterfly and sqrt per step
      show most).

Sides, closed form on every one: simulate_alg_curve([T]) (the yardstick: one curve pass, the
machine code of the commit before the anytime kernels), simulate_alg_anytime with K = 1 and
K = 10 without the trace and, in (a) and (b), K = 1 with the trace (which includes the un-tiling
copy); in (a) also simulate_alg_curve at K = 100, from which the dense curve the anytime form
replaces is extrapolated linearly to K = T (the curve's cost is linear in K).

One process; device events around every repetition; every side warmed up; the sides alternate
repetition by repetition, so all see the same neighbours on the machine.  Each ratio comes with
the spread of both of its sides.  --small runs toy sizes (a rehearsal of the script, not a
measurement)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_convex_optimization_amd import engine  # noqa: E402

ETA0 = math.sqrt(2)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(sides, reps, warm=3):
    """{name: [ms] * reps}, the sides taking turns."""
    for _ in range(warm):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            ms[k].append(timed(fn))
    return ms


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
            "stdev_ms": statistics.pstdev(v), "reps": len(v)}


def case(out, name, B, T, d, reps, with_trace, with_k100):
    db = engine.DeviceBatch(B, T, d).generate_gT(base_seed=0)
    k10 = list(range(T // 10, T + 1, T // 10))
    res = {}

    def curve(ck, key):
        return lambda: res.__setitem__(key, db.simulate_alg_curve(ck, 0, ETA0,
                                                                  closed_comparator=True))

    def anytime(ck, key, trace=False):
        return lambda: res.__setitem__(key, db.simulate_alg_anytime(ck, 0, ETA0,
                                                                    closed_comparator=True,
                                                                    trace=trace))

    sides = {"curve_K1": curve([T], "curve_K1"), "anytime_K1": anytime([T], "anytime_K1"),
             "anytime_K10": anytime(k10, "anytime_K10")}
    if with_trace:
        sides["anytime_K1_trace"] = anytime([T], "anytime_K1_trace", trace=True)
    if with_k100:
        sides["curve_K100"] = curve(list(range(T // 100, T + 1, T // 100)), "curve_K100")
    ms = alternate(sides, reps)
    st = {k: stats(v) for k, v in ms.items()}
    base = st["curve_K1"]
    rec = {"case": name, "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
           "sides": st,
           "ratio_median": {k: s["median_ms"] / base["median_ms"] for k, s in st.items()},
           "all_certified": bool((res["anytime_K1"]["open_from"] == T + 1).all().item()),
           # sup >= the regret at T, and the two anytime lists agree on the last horizon
           "sup_bounds_curve": bool((res["anytime_K1"]["sup"][:, 0]
                                     >= res["curve_K1"]["regret"][:, 0]).all().item()),
           "K10_last_equals_K1": bool(torch.equal(res["anytime_K10"]["sup"][:, -1],
                                                  res["anytime_K1"]["sup"][:, 0]))}
    if with_trace:
        tr = res["anytime_K1_trace"]["trace"]
        rec["trace_last_equals_curve"] = bool(torch.equal(tr[:, -1],
                                                          res["curve_K1"]["regret"][:, 0]))
        rec["trace_max_equals_sup"] = bool(torch.equal(tr.max(dim=1).values,
                                                       res["anytime_K1"]["sup"][:, 0]))
    if with_k100:
        per_ck = (st["curve_K100"]["median_ms"] - base["median_ms"]) / 99.0
        rec["dense_curve_extrapolated_ms"] = base["median_ms"] + per_ck * (T - 1)
        rec["curve_ms_per_checkpoint"] = per_ck
    out(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "anytime_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cases", default="abc")
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
    shapes = {"a": (4096, 1000, 64) if a.small else (32768, 10000, 64),
              "b": (4096, 200, 5) if a.small else (65536, 1000, 5),
              "c": (512, 2000, 64) if a.small else (4900, 100000, 64)}
    for name in "abc":
        if name in a.cases:
            case(out, name, *shapes[name], a.reps, with_trace=name != "c", with_k100=name == "a")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
