"""FTRL-vs-exact-FTL regret-grid timing probe: one DeviceBatch.ftrl_vs_exact_curve_etas call for
M step sizes x K = 10 horizons against the M DeviceBatch.ftrl_vs_exact_curve calls it replaces
(that code is unchanged), on resident generate_gT batches.  One JSON line per (shape, M),
appended to profiles/exact_grid_ab.jsonl (or --out).

Shapes (name: B x T x d, lanes_per_seq, closed comparator):
  bench    32 768 x 1e4 x 64, default layout, closed form (the bench layout)
  mid       4 096 x 1e4 x 64, default layout, closed form
  exact5   65 536 x 1e3 x 5, exact mode: every pair streams
  and one shape per further layout class that has a multi-column instance (c2, c4: butterfly
  sums at 2 and 4 coordinates per lane; chain8, chain4: chained sums).

The grid is timed with the dispatcher's group and with every group the layout has an instance
for (forced), so one run shows which group a layout class should take.  One process; device
events on the batch's stream around every repetition; every shape warmed up; the sides take
turns repetition by repetition, so all see the same neighbours on the machine.  Before the
timed region, once per shape, every output of every timed grid configuration is compared bit
for bit with the M curve calls.  --small runs toy sizes (a rehearsal of the script, not a
measurement)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_convex_optimization_amd import _lib, engine  # noqa: E402

ETAS = [1.0, math.sqrt(2), 2.0, 0.5]
SHAPES = {   # B, T, d, lanes_per_seq, closed comparator
    "bench": (32768, 10000, 64, engine.LANES_BEST, True),
    "mid": (4096, 10000, 64, engine.LANES_BEST, True),
    "exact5": (65536, 1000, 5, 1, False),
    "c2": (65536, 5000, 16, 8, True),
    "c4": (32768, 5000, 32, 8, True),
    "chain8": (8192, 10000, 64, -8, True),
    "chain4": (32768, 5000, 16, -4, True),
}
THREE = ("cum_ftrl", "comp_ftl", "ftrl")


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


def offered(L):
    """The groups the layout has an instance for: the argument check of an empty call."""
    f = _lib.load().ocx_dev_ftrl_vs_exact_curve_etas
    buf = ctypes.c_void_p(16)   # never dereferenced: M = 0
    return [g for g in (1, 2, 4)
            if f(ctypes.byref(L), buf, buf, None, 0, None, 0, None, None, None, None, None,
                 None, None, 0, 0, g, None, 0, None) == 0]


def bits_equal(grid, calls):
    """Every output of a grid result against the M curve results, bit for bit."""
    ok = True
    for m, ref in enumerate(calls):
        for k, v in ref.items():
            g = grid[k][:, m] if k in THREE else grid[k]
            ok = ok and bool(torch.equal(g, v))
    return ok


def shape_case(out, name, B, T, d, lanes, closed, reps):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes).generate_gT(base_seed=0)
    cks = list(range(T // 10, T + 1, T // 10))
    kw = dict(closed_comparator=closed)
    groups = offered(db.L)
    auto = int(_lib.load().ocx_ftrl_exact_grid_group(ctypes.byref(db.L)))
    for M in (2, 4):
        etas = ETAS[:M]
        calls = [db.ftrl_vs_exact_curve(cks, e, **kw) for e in etas]
        use = [g for g in groups if g == 1 or g // 2 < M]
        equal = {f"g{g}": bits_equal(db.ftrl_vs_exact_curve_etas(cks, etas, _group=g, **kw), calls)
                 for g in use}
        first = db.ftrl_vs_exact_curve_etas(cks, etas, **kw)
        equal["auto"] = bits_equal(first, calls)
        torch.cuda.synchronize()
        assert all(equal.values()), (name, M, equal)
        closed_share = float((first["closed"] == 1).double().mean().item())
        del calls, first
        res = {}

        def m_calls():
            for e in etas:
                res["c"] = db.ftrl_vs_exact_curve(cks, e, **kw)

        sides = {"calls": m_calls}
        for g in use:
            sides[f"g{g}"] = (lambda g=g: res.__setitem__(
                "g", db.ftrl_vs_exact_curve_etas(cks, etas, _group=g, **kw)))
        ms = alternate(sides, reps)
        st = {k: stats(v) for k, v in ms.items()}
        base = st["calls"]
        rec = {"shape": name, "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
               "closed_comparator": closed, "closed_share": closed_share, "M": M, "K": len(cks),
               "auto_group": auto, "bits_equal": equal, "calls": base}
        for g in use:
            s = st[f"g{g}"]
            spread = (s["max_ms"] - s["min_ms"]) + (base["max_ms"] - base["min_ms"])
            rec[f"g{g}"] = dict(s, ratio_to_calls=s["median_ms"] / base["median_ms"],
                                gain_ms=base["median_ms"] - s["median_ms"],
                                combined_spread_ms=spread,
                                faster=base["median_ms"] - s["median_ms"] > spread)
        out(rec)
        res.clear()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "exact_grid_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def out(rec):
        rec["small"] = a.small
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    for name in a.shapes.split(","):
        B, T, d, lanes, closed = SHAPES[name]
        if a.small:
            B, T = max(B // 64, 64), max(T // 10, 100)
        engine.release_buffers(0)
        torch.cuda.empty_cache()
        shape_case(out, name, B, T, d, lanes, closed, a.reps)


if __name__ == "__main__":
    main()
