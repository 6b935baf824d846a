"""FTRL-vs-exact-FTL regret-curve timing probe: what observing K checkpoint horizons in one pass
(DeviceBatch.ftrl_vs_exact_curve) costs next to the unchanged single-horizon kernel
(DeviceBatch.ftrl_vs_exact) in the same library, on resident generate_gT batches.  One JSON
line per case, appended to profiles/exact_curve_ab.jsonl (or --out).

  (a) 32 768 x 1e4 x 64, default layout (OCX_LANES_BEST), closed form, K = 10 (1000 .. 10000)
      and K = 100: against ONE ftrl_vs_exact() at full T; and, for K = 10, against the ten
      ftrl_vs_exact() calls on resident truncated batches — at 4 096 sequences, both sides:
      the ten truncated batches hold 5.5 x the batch's rows and do not fit beside it;
  (b) 65 536 x 1e3 x 5 in exact mode (streamed comparator for every pair), ten horizons
      100 .. 1000: one curve call against the ten truncated calls.

One process; device events on the batch's stream around every repetition; every shape warmed
up; the sides of a comparison alternate repetition by repetition, so both see the same
neighbours on the machine.  --small runs toy sizes (a rehearsal of the script, not a
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


def truncated_batches(db, cks, lanes, chunk=4096):
    """Resident batches of the first t rows of db for every t of cks (the same layout), packed
    from a few thousand sequences' rows at a time."""
    B, d = db.L.B, db.L.d
    zs = [torch.empty((B, t, d), dtype=torch.float64, device=db.device) for t in cks]
    ys = [torch.empty((B, t), dtype=torch.float64, device=db.device) for t in cks]
    for b0 in range(0, B, chunk):
        seqs = torch.arange(b0, min(B, b0 + chunk), device=db.device)
        z, y = db.rows_of(seqs)
        for i, t in enumerate(cks):
            zs[i][b0:b0 + chunk] = z[:, :t]
            ys[i][b0:b0 + chunk] = y[:, :t]
        del z, y
    out = []
    for i, t in enumerate(cks):
        out.append(engine.DeviceBatch(B, t, d, lanes_per_seq=lanes).pack(zs[i], ys[i]))
        torch.cuda.synchronize()
        zs[i] = ys[i] = None
        out[-1]._keep = None
        torch.cuda.empty_cache()
    return out


def columns_equal(res, trunc, B):
    """Column k of the curve against the truncated batches' last ftrl_vs_exact() results."""
    return all(bool(torch.equal(res["cum_ftrl"][:, k], t.cum[:B])
                    and torch.equal(res["cum_exact"][:, k], t.cum_exact[:B])
                    and torch.equal(res["comp"][:, k], t.comp[:B]))
               for k, t in enumerate(trunc))


def case_a(out, B, T, d, trunc_div, reps):
    db = engine.DeviceBatch(B, T, d).generate_gT(base_seed=0)
    lists = {"K10": list(range(T // 10, T + 1, T // 10)),
             "K100": list(range(T // 100, T + 1, T // 100))}
    res = {}
    sides = {"single": lambda: db.ftrl_vs_exact(ETA0, closed_comparator=True)}
    for name, ck in lists.items():
        sides[name] = (lambda ck=ck, name=name: res.__setitem__(
            name, db.ftrl_vs_exact_curve(ck, ETA0, closed_comparator=True)))
    ms = alternate(sides, reps)
    base = stats(ms["single"])
    for name, ck in lists.items():
        s = stats(ms[name])
        out({"case": "a", "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
             "K": len(ck), "single": base, "curve": s,
             "ratio_to_single": s["median_ms"] / base["median_ms"],
             "inside_single_spread": base["min_ms"] <= s["median_ms"] <= base["max_ms"],
             "all_closed": bool((res[name]["closed"] == 1).all().item()),
             "last_column_equals_single": bool(torch.equal(res[name]["comp"][:, -1],
                                                           db.comp[:B]))})
    # against the K truncated calls: the ten truncated batches hold 5.5 x the batch's rows and
    # do not fit beside it at full size, so this comparison runs at B / trunc_div sequences,
    # both sides; the truncated batches are generate_gT batches of their own horizon (the
    # closed-form path's time does not depend on the rows)
    del db, sides
    res.clear()
    torch.cuda.empty_cache()
    Bs = B // trunc_div
    ds = engine.DeviceBatch(Bs, T, d).generate_gT(base_seed=0)
    trunc = [engine.DeviceBatch(Bs, t, d).generate_gT(base_seed=0) for t in lists["K10"]]
    assert all((t.L.P, t.L.C, t.L.chain) == (ds.L.P, ds.L.C, ds.L.chain) for t in trunc)

    def k_truncated():
        for t in trunc:
            t.ftrl_vs_exact(ETA0, closed_comparator=True)

    ms = alternate({"K10_truncated": k_truncated,
                    "K10": lambda: res.__setitem__("c", ds.ftrl_vs_exact_curve(
                        lists["K10"], ETA0, closed_comparator=True)),
                    "single": lambda: ds.ftrl_vs_exact(ETA0, closed_comparator=True)}, reps)
    ten, s, one = stats(ms["K10_truncated"]), stats(ms["K10"]), stats(ms["single"])
    out({"case": "a_truncated", "B": Bs, "T": T, "d": d, "layout": [ds.L.P, ds.L.C, ds.L.chain],
         "K": 10, "K_truncated": ten, "curve": s, "single": one,
         "ratio_to_K_truncated": s["median_ms"] / ten["median_ms"],
         "ratio_to_single": s["median_ms"] / one["median_ms"],
         "all_closed": bool((res["c"]["closed"] == 1).all().item())})


def case_b(out, B, d, reps):
    cks = list(range(100, 1100, 100))
    T = cks[-1]
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=1).generate_gT(base_seed=0)
    trunc = truncated_batches(db, cks, 1, chunk=16384)
    res = {}

    def ten():
        for t in trunc:
            t.ftrl_vs_exact(ETA0)

    ms = alternate({"ten_truncated": ten,
                    "curve": lambda: res.__setitem__("c", db.ftrl_vs_exact_curve(cks, ETA0))},
                   reps)
    base, s = stats(ms["ten_truncated"]), stats(ms["curve"])
    out({"case": "b", "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
         "K": len(cks), "ten_truncated": base, "curve": s,
         "ratio_to_K_truncated": s["median_ms"] / base["median_ms"],
         "none_closed": bool((res["c"]["closed"] == 0).all().item()),
         "columns_bit_equal": columns_equal(res["c"], trunc, B)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "exact_curve_ab.jsonl"))
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
        case_a(out, *((4096, 1000, 64, 2) if a.small else (32768, 10000, 64, 8)), a.reps)
        torch.cuda.empty_cache()
    if "b" in a.cases:
        case_b(out, 4096 if a.small else 65536, 5, a.reps)


if __name__ == "__main__":
    main()
