"""Step-size sweep timing probe: what M step sizes cost through simulate_alg_etas, for every
forced group size, next to M separate calls of the existing single-eta path on the same
resident data.  One JSON line per case, appended to profiles/etas_ab.jsonl (or --out).

  (a) the generate_gT batch 32 768 x 1e4 x 64 (OCX_LANES_BEST), closed form on both sides:
      M x simulate_alg() against simulate_alg_etas with M in {1, 2, 4, 8}, group in {1, 2, 4}
      (forced through include/ocx_testing.h) and the dispatcher's own choice;
  (b) the same at 65 536 x 1e3 x 5 and 65 536 x 1e3 x 16;
  (c) gT_regrets_etas(1e4, 32 768, 4 step sizes, d = 64) against four gT_regrets calls;
  (d) M in {2, 4} on further layout classes the default modes choose (see main()).

The baseline is always the existing code, never the sweep code.  One process; device events
on the batch's stream around every repetition; every shape warmed up; the sides of a comparison
alternate repetition by repetition, so both see the same neighbours on the machine.  (c) is
timed with a host clock around synchronous calls, and its two sides run one after the other:
each keeps a batch of 170 GB resident, and the two do not fit side by side.  The spread
reported is that of the existing path in the same call.  --small runs toy sizes (a rehearsal
of the script, not a measurement)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_convex_optimization_amd import _lib, engine  # noqa: E402

SQ2 = math.sqrt(2)
ETAS8 = [SQ2, 0.25, 1.0, 2.0, 8.0, 0.5, 4.0, 1.5]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(sides, reps, warm=2):
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


def resident(out, case, B, T, d, reps, lanes=engine.LANES_BEST, Ms=(1, 2, 4, 8)):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes).generate_gT(base_seed=0)
    cc = not db.exact   # both sides: the batch's default comparator
    groups = [g for g in (1, 2, 4) if g == 1 or db.L.C <= 8 or (g == 2 and db.L.C <= 16)]
    for M in Ms:
        etas = ETAS8[:M]
        res = {}

        def loop(etas=etas):
            for eta in etas:
                db.simulate_alg(0, eta, closed_comparator=cc)

        sides = {"loop": loop}
        for g in groups + [None]:
            name = "auto" if g is None else f"group{g}"
            sides[name] = (lambda g=g, name=name, etas=etas: res.__setitem__(
                name, db.simulate_alg_etas(etas, closed_comparator=cc, _group=g)))
        ms = alternate(sides, reps)
        base = stats(ms["loop"])
        torch.cuda.synchronize()   # db.regret holds the last step size's run
        rec = {"case": case, "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
               "closed_comparator": cc, "M": M, "auto_group": int(_lib.load().ocx_etas_group(ctypes.byref(db.L), M)),
               "loop": base}
        for name in sides:
            if name == "loop":
                continue
            s = stats(ms[name])
            rec[name] = dict(s, ratio_median=s["median_ms"] / base["median_ms"],
                             inside_loop_spread=base["min_ms"] <= s["median_ms"] <= base["max_ms"],
                             last_column_equals_simulate_alg=bool(
                                 torch.equal(res[name]["regret"][:, -1], db.regret[:B])))
        out(rec)
    del db


def case_c(out, T, runs, d, reps):
    etas = ETAS8[:4]

    def host_timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def four():
        return np.stack([engine.gT_regrets(T, runs, d=d, eta0=eta) for eta in etas], axis=1)

    def sweep():
        return engine.gT_regrets_etas(T, runs, etas, d=d, return_closed=True)

    host_timed(four)   # warm-up: the library's buffers
    a = [host_timed(four) for _ in range(reps)]
    engine.release_buffers(0)
    host_timed(sweep)  # warm-up: the caching allocator's blocks
    b = [host_timed(sweep) for _ in range(reps)]
    ref, (got, closed) = a[-1][1], b[-1][1]
    base, s = stats([x[0] for x in a]), stats([x[0] for x in b])
    L = _lib.layout(runs, T, d, engine.LANES_BEST)
    out({"case": "c", "runs": runs, "T": T, "d": d, "layout": [L.P, L.C, L.chain], "M": 4,
         "auto_group": int(_lib.load().ocx_etas_group(ctypes.byref(L), 4)), "four_gT_regrets": base,
         "gT_regrets_etas": s, "ratio_median": s["median_ms"] / base["median_ms"],
         "all_closed": bool((closed == 1).all()),
         "max_abs_diff": float(np.max(np.abs(got - ref))) if got.size else 0.0})
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "etas_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cases", default="cabd")
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
    if "c" in a.cases:
        case_c(out, *((1000, 4096, 64) if a.small else (10000, 32768, 64)), max(3, a.reps // 2))
    if "a" in a.cases:
        resident(out, "a", *((4096, 1000, 64) if a.small else (32768, 10000, 64)), a.reps)
        torch.cuda.empty_cache()
    if "b" in a.cases:
        for d in (5, 16):
            resident(out, "b", 4096 if a.small else 65536, 100 if a.small else 1000, d, a.reps)
            torch.cuda.empty_cache()
    if "d" in a.cases:
        # further members of the dispatcher's classes (loop form x coordinates per lane):
        # pipelined 16 x 4 (few-wave long horizons), 8 x 4, 32 x 8 and 16 x 16; chained 2 x 16
        # (d = 32), 4 x 16 (the bit-exact mode at d = 64, two-pass comparator), 4 x 2 and the
        # few-wave 8 x 8 chain; butterfly lanes the pipelined form does not take (2 x 4);
        # one lane of 12 coordinates
        extra = [(3328, 100000, 64, 128), (65536, 5000, 32, 8), (8192, 5000, 256, 32),
                 (8192, 10000, 200, 128), (65536, 1000, 32, 128), (32768, 10000, 64, 1),
                 (65536, 1000, 5, -4), (4900, 20000, 64, 1), (65536, 1000, 5, 2),
                 (65536, 1000, 12, -1)]
        if a.small:
            extra = [(B // 16, T // 50, d, lanes) for B, T, d, lanes in extra]
        for B, T, d, lanes in extra:
            resident(out, "d", B, T, d, a.reps, lanes, (2, 4))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
