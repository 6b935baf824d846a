"""Regret-curve timing probe: what observing K checkpoint horizons in one pass costs next to the
existing single-horizon kernels, on resident batches.  One JSON line per case, appended to
profiles/curve_ab.jsonl (or --out).

  (a) the generate_gT batch 32 768 x 1e4 x 64 (OCX_LANES_BEST), closed form on both sides:
      simulate_alg() against simulate_alg_curve with K = 10 (1000 .. 10000) and K = 100;
  (b) the reference's grid at d = 5: 65 536 sequences, checkpoints 100 .. 1000, exact mode:
      one curve call against ten truncated simulate_alg calls on resident data.

One process; device events on the batch's stream around every repetition; every shape warmed
up; the sides of a comparison alternate repetition by repetition, so both see the same
neighbours on the machine.  The spread reported is that of the existing kernel in the same
call.  --small runs toy sizes (a rehearsal of the script, not a measurement)."""
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


def case_a(out, B, T, d, reps):
    db = engine.DeviceBatch(B, T, d).generate_gT(base_seed=0)
    lists = {"K10": list(range(T // 10, T + 1, T // 10)),
             "K100": list(range(T // 100, T + 1, T // 100))}
    res = {}
    sides = {"simulate_alg": lambda: db.simulate_alg(0, ETA0, closed_comparator=True)}
    for name, ck in lists.items():
        sides[name] = (lambda ck=ck, name=name:
                       res.__setitem__(name, db.simulate_alg_curve(ck, 0, ETA0,
                                                                   closed_comparator=True)))
    ms = alternate(sides, reps)
    base = stats(ms["simulate_alg"])
    same = {k: bool(torch.equal(res[k]["regret"][:, -1], db.regret[:B])) for k in lists}
    closed = {k: bool((res[k]["closed"] == 1).all().item()) for k in lists}
    for name in lists:
        s = stats(ms[name])
        out({"case": "a", "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
             "K": len(lists[name]), "simulate_alg": base, "curve": s,
             "ratio_median": s["median_ms"] / base["median_ms"],
             "inside_spread": base["min_ms"] <= s["median_ms"] <= base["max_ms"],
             "last_column_equals_simulate_alg": same[name], "all_closed": closed[name]})


def case_b(out, B, d, reps):
    cks = list(range(100, 1100, 100))
    T = cks[-1]
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=1).generate_gT(base_seed=0)
    # the ten truncated runs' resident data: the same rows, packed per horizon
    seqs = torch.arange(B, device=db.device)
    z, y = db.rows_of(seqs)
    trunc = [engine.DeviceBatch(B, t, d, lanes_per_seq=1).pack(z[:, :t].contiguous(),
                                                               y[:, :t].contiguous())
             for t in cks]
    del z, y
    res = {}

    def ten():
        for t in trunc:
            t.simulate_alg(0, ETA0)

    ms = alternate({"ten_truncated": ten,
                    "curve": lambda: res.__setitem__("c", db.simulate_alg_curve(cks, 0, ETA0))},
                   reps)
    same = all(bool(torch.equal(res["c"]["regret"][:, k], t.regret[:B]))
               for k, t in enumerate(trunc))
    base, s = stats(ms["ten_truncated"]), stats(ms["curve"])
    out({"case": "b", "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
         "K": len(cks), "ten_truncated": base, "curve": s,
         "ratio_median": s["median_ms"] / base["median_ms"], "columns_bit_equal": same})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "curve_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cases", default="ab")
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
    if "a" in a.cases:
        case_a(out, *((4096, 1000, 64) if a.small else (32768, 10000, 64)), a.reps)
        torch.cuda.empty_cache()
    if "b" in a.cases:
        case_b(out, 4096 if a.small else 65536, 5, a.reps)


if __name__ == "__main__":
    main()
